"""GPU tests of the checkpoint archive (include/npp_amd.h npp_archive_create, nclone_amd/csrc/npp_archive.hip): a
state stored from one env restores into ANY env of the same level and continues the source's future bit for bit; it equals what the
reference's "reset + replay the action sequence" reaches; the reachability cache travels with it; the per-entry status is decided
on the device and only status 0 touches an env; the refusals; the meta rows; the observation overlap is joined; the host classes.
The base shape: 192 envs, blocks 0 and 2 on level 0 and block 1 on level 1, 8 slots."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, SLOTS = 192, 8
LEVEL_IDS = (np.arange(N) // 64) % 2
SRC_ENVS, SRC_SLOTS = [3, 70, 130], [5, 0, 2]            # stored: level 0, level 1, level 0
DST_ENVS, DST_SLOTS, DST_SRC = [10, 150, 100], [5, 5, 0], [3, 3, 70]   # same block, other block of the same level, level 1
REACH_OUT = ("positions", "reachability_features", "mine_sdf_features", "reach_status")


def _levels(which):
    from nclone_amd import levels as lv

    return getattr(lv, which + "_levels")()[0][:2]


def _reach_levels():
    z = np.load(os.path.join(ROOT, "tests", "golden", "reach.npz"))
    names = bytes(z["names"]).decode().split("\n")
    miss = {"doors:hcorr:door:100053", "mines:hcorr:mines:100025", "c0:replay:20", "c0:replay:63", "c0:replay:68", "c0:replay:78",
            "mines:hcorr:mines:100008"}   # (tests/test_gpu_reach.py MISS_BRANCH)
    sup = [k for k, n in enumerate(names) if n not in miss]
    return [np.ascontiguousarray(z["m%d" % k]) for k in sup[:2]]


def _batch(levels, outputs=(), autoreset=True, n=N, level_ids=LEVEL_IDS, slots=SLOTS):
    from nclone_amd.engine import NppBatch

    b = NppBatch(n, autoreset=autoreset, outputs=outputs)
    b.load_levels(levels)
    b.assign_levels(level_ids)
    if slots:
        b.archive_create(slots)
    return b


def _acts(seed, steps, n=N):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 6, size=(steps, n)).astype(np.uint8)).cuda()


def _full(b, envs=None):
    """Everything the parity hooks show of the given envs (all by default)."""
    f, i = b.dump_state()
    cs = b.entity_checksum()
    envs = range(b.n) if envs is None else envs
    return {"f": f, "i": i, "cs": cs, "ent": {int(e): b.dump_entities(int(e)) for e in envs}}


def _rows_equal(a, ea, b, eb):
    return (np.array_equal(a["f"][ea], b["f"][eb]) and np.array_equal(a["i"][ea], b["i"][eb]) and
            np.array_equal(a["cs"][ea], b["cs"][eb], equal_nan=True) and np.array_equal(a["ent"][ea], b["ent"][eb]))


def _status(t):
    return t.cpu().numpy().tolist()


def _cross_env(levels, overlap=0, direct=False):
    """Store three envs after 20 steps; restore two slots into three other envs; follow the sources' recorded actions.
    direct: one step between store and restore and nothing (no dump, no join) between that step and the restore -- the form the
    observation-overlap test compares with and without the overlap; returns what the parity hooks show afterwards."""
    b = _batch(levels, outputs=("spatial_context",))
    b.set_step_variant(0)   # (a pinned build: a split step needs no autotuner decision first; same bits)
    if overlap:
        b.set_obs_overlap(overlap)
    acts = _acts(5, 35)
    for t in range(20):
        b.step(acts[t])
    assert _status(b.archive_store(SRC_ENVS, SRC_SLOTS, status=True)) == [0, 0, 0]
    at_store = _full(b)
    if direct:
        b.step(acts[20])
        assert _status(b.archive_restore(DST_ENVS, DST_SLOTS, status=True)) == [0, 0, 0]
        after = _full(b)
        for dst, src in zip(DST_ENVS, DST_SRC):
            assert _rows_equal(after, dst, at_store, src), (dst, src)
        for t in range(21, 35):
            b.step(acts[t])
        later = _full(b)
        out = {"after": after, "later": later, "sc": b.spatial_context.cpu().numpy().copy()}
        b.close()
        return out
    for t in range(20, 35):
        b.step(acts[t])
    src_later = _full(b)
    src_sc = b.spatial_context.cpu().numpy().copy()
    assert not np.array_equal(src_later["f"][SRC_ENVS], at_store["f"][SRC_ENVS])
    assert _status(b.archive_restore(DST_ENVS, DST_SLOTS, status=True)) == [0, 0, 0]
    after = _full(b)
    for dst, src in zip(DST_ENVS, DST_SRC):
        assert _rows_equal(after, dst, at_store, src), (dst, src)
    for e in range(N):   # envs outside the lists: bit-identical before and after the restore call
        if e not in DST_ENVS:
            assert _rows_equal(after, e, src_later, e), e
    # the targets are fed their sources' recorded actions: they reach the sources' rows after those steps
    replay = acts[20:35].clone()
    for dst, src in zip(DST_ENVS, DST_SRC):
        replay[:, dst] = acts[20:35, src]
    for t in range(15):
        b.step(replay[t])
    dst_later = _full(b, DST_ENVS)
    dst_sc = b.spatial_context.cpu().numpy()
    for dst, src in zip(DST_ENVS, DST_SRC):
        assert _rows_equal(dst_later, dst, src_later, src), (dst, src)
        assert np.array_equal(dst_sc[dst], src_sc[src]), (dst, src)
    b.close()


@pytest.mark.parametrize("which", ["mine", "door", "zoo"])
def test_cross_env_restore_continues_the_sources_future(which):
    _cross_env(_levels(which))


def test_restored_state_is_reset_plus_replay():
    """The reference's definition of a checkpoint (base_environment.py:1769-1789): reset, then replay the action sequence."""
    b = _batch(_levels("mine"), autoreset=False)
    b.set_truncation_limit(10000)
    b.reset()
    acts = _acts(21, 20)
    for t in range(20):
        b.step(acts[t])
    assert _status(b.archive_store([3, 70], [5, 0], status=True)) == [0, 0]
    b.reset()
    assert _status(b.archive_restore([10, 100], [5, 0], status=True)) == [0, 0]
    restored = _full(b, [10, 100])
    replay = acts.clone()
    replay[:, 11] = acts[:, 3]
    replay[:, 101] = acts[:, 70]
    for t in range(20):
        b.step(replay[t])
    replayed = _full(b, [11, 101])
    assert _rows_equal(replayed, 11, restored, 10) and _rows_equal(replayed, 101, restored, 100)
    assert restored["i"][10, 22] > 0
    b.close()


def test_reachability_cache_travels_with_the_record():
    levels = _reach_levels()
    b = _batch(levels, outputs=REACH_OUT)
    b.reset()
    acts = _acts(3, 40)
    for t in range(30):
        b.step(acts[t])
        b.reachability()
    assert _status(b.archive_store(SRC_ENVS, SRC_SLOTS, status=True)) == [0, 0, 0]
    rec = [{k: v.copy() for k, v in b.to_host(REACH_OUT).items()}]
    for t in range(30, 40):
        b.step(acts[t])
        b.reachability()
        rec.append({k: v.copy() for k, v in b.to_host(REACH_OUT).items()})
    assert _status(b.archive_restore(DST_ENVS, DST_SLOTS, status=True)) == [0, 0, 0]
    b.observe()
    b.reachability()
    replay = acts[30:40].clone()
    for dst, src in zip(DST_ENVS, DST_SRC):
        replay[:, dst] = acts[30:40, src]
    for t in range(11):
        h = b.to_host(REACH_OUT)
        for dst, src in zip(DST_ENVS, DST_SRC):
            for k in REACH_OUT:
                assert np.array_equal(h[k][dst], rec[t][k][src]), (t, dst, k)
        if t < 10:
            b.step(replay[t])
            b.reachability()
    b.close()
    # a slot stored before the first npp_reachability: the restored env has no cached vector, recomputes, and agrees
    b = _batch(levels, outputs=REACH_OUT)
    b.reset()
    for t in range(12):
        b.step(acts[t])
    assert _status(b.archive_store([3], [1], status=True)) == [0]
    b.reachability()
    before = {k: v.copy() for k, v in b.to_host(REACH_OUT).items()}
    assert not np.array_equal(before["positions"][10], before["positions"][3])
    assert _status(b.archive_restore([10, 150], [1, 1], status=True)) == [0, 0]
    b.observe()
    b.reachability()
    h = b.to_host(REACH_OUT)
    for dst in (10, 150):
        for k in REACH_OUT:
            assert np.array_equal(h[k][dst], before[k][3]), (dst, k)
    for k in REACH_OUT:   # the others keep their rows
        keep = np.setdiff1d(np.arange(N), [10, 150])
        assert np.array_equal(h[k][keep], before[k][keep]), k
    b.close()


def test_status_codes_and_refusals():
    from nclone_amd import _native as nat

    levels = _levels("mine")
    b = _batch(levels, slots=0)

    def refused(fn, *args, match):
        with pytest.raises(nat.NppError, match=match) as ei:
            fn(*args)
        assert ei.value.code == nat.NPP_ERR_STATE

    refused(b.archive_store, [3], [5], match="no archive")
    refused(b.archive_restore, [3], [5], match="no archive")
    with pytest.raises(nat.NppError) as ei:
        nat.check(b.h, b.lib.npp_archive_create(b.h, -1))
    assert ei.value.code == nat.NPP_ERR_INVALID
    b.archive_create(SLOTS)
    assert b.archive_num_slots() == SLOTS and b.archive_record_bytes() > 0 and b.archive_record_bytes() % 16 == 0
    acts = _acts(9, 8)
    for t in range(8):
        b.step(acts[t])
    assert _status(b.archive_store([3], [5], status=True)) == [0]
    before = _full(b)
    # level mismatch (a level-0 slot into env 70), an empty slot, slot == n_slots, env == n_envs, a skipped entry, a valid one
    st = b.archive_restore([70, 10, 11, N, -1, 12], [5, 6, SLOTS, 5, 5, 5], status=True)
    assert _status(st) == [2, 3, 4, 4, 1, 0]
    after = _full(b)
    for e in range(N):
        assert _rows_equal(after, e, before, 3 if e == 12 else e), e
    assert _status(b.archive_store([4, N, 5, -1], [SLOTS, 1, -1, 1], status=True)) == [4, 4, 1, 1]
    assert b.archive_meta()["stored"].cpu().numpy().tolist() == [0, 0, 0, 0, 0, 1, 0, 0]
    # assign_levels keeps the archive; the device sees that env 10 now plays level 1
    b.assign_levels(np.array([1], dtype=np.int32), env_ids=np.array([10], dtype=np.int32))
    assert _status(b.archive_restore([10, 11], [5, 5], status=True)) == [2, 0]
    # while an archive exists the pool and a repositioning are refused; with either on, there is no archive to be had
    refused(b.set_level_pool, [1.0, 1.0], 7, match="checkpoint archive exists")
    refused(b.set_entity_pos, 0, 0, 300.0, 300.0, match="checkpoint archive exists")
    b.archive_create(0)
    assert b.archive_num_slots() == 0
    b.set_level_pool([1.0, 1.0], 7)
    refused(b.archive_create, SLOTS, match="level pool is on")
    b.set_level_pool(None)
    b.set_entity_pos(0, 0, 300.0, 300.0)
    refused(b.archive_create, SLOTS, match="repositioned")
    b.set_entity_pos(0, 0, float("nan"), float("nan"))
    b.archive_create(SLOTS)
    assert _status(b.archive_store([3], [5], status=True)) == [0]
    # npp_load_levels drops the archive
    b.load_levels(levels)
    assert b.archive_num_slots() == 0
    refused(b.archive_restore, [3], [5], match="no archive")
    b.close()


def test_meta_rows():
    b = _batch(_levels("door"))
    acts = _acts(13, 25)
    for t in range(25):
        b.step(acts[t])
    assert _status(b.archive_store(SRC_ENVS, SRC_SLOTS, status=True)) == [0, 0, 0]
    f, i = b.dump_state()
    m = {k: v.cpu().numpy() for k, v in b.archive_meta().items()}
    assert m["x"].dtype == np.float64 and m["frame"].dtype == np.int32 and all(len(v) == SLOTS for v in m.values())
    stored = np.zeros(SLOTS, dtype=np.int32)
    stored[SRC_SLOTS] = 1
    assert np.array_equal(m["stored"], stored)
    for c, k in enumerate(("x", "y", "vx", "vy")):
        assert np.array_equal(m[k][SRC_SLOTS], f[SRC_ENVS, c]), k
    assert np.array_equal(m["level"][SRC_SLOTS], LEVEL_IDS[SRC_ENVS]) and np.array_equal(m["level"][SRC_SLOTS], i[SRC_ENVS, 27])
    assert np.array_equal(m["frame"][SRC_SLOTS], i[SRC_ENVS, 22])
    assert np.array_equal(m["cell_x"][SRC_SLOTS], np.floor(f[SRC_ENVS, 0] / 24).astype(np.int32))
    assert np.array_equal(m["cell_y"][SRC_SLOTS], np.floor(f[SRC_ENVS, 1] / 24).astype(np.int32))
    assert np.array_equal(m["switch_activated"][SRC_SLOTS], (i[SRC_ENVS, 13] != 1).astype(np.int32))
    # the views stay valid: a later store shows in them without another call
    view = b.archive_meta()["stored"]
    assert _status(b.archive_store([20], [7], status=True)) == [0]
    assert view.cpu().numpy()[7] == 1
    b.close()


def test_restore_joins_an_observation_overlap():
    levels = _levels("mine")
    plain = _cross_env(levels, overlap=0, direct=True)
    split = _cross_env(levels, overlap=40, direct=True)
    for k in ("after", "later"):
        for e in range(N):
            assert _rows_equal(plain[k], e, split[k], e), (k, e)
    assert np.array_equal(plain["sc"], split["sc"])


def _copy_obs(obs):
    return {k: (v.clone() if isinstance(v, torch.Tensor) else np.array(v, copy=True)) for k, v in obs.items()}


def _np(v):
    return v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def _slot_ids(pairs):
    s = np.full(N, -1, dtype=np.int32)
    for e, slot in pairs:
        s[e] = slot
    return s


@pytest.mark.parametrize("output", ["torch", "numpy"])
def test_vec_env_checkpoint_reset_repads_the_stacks(output):
    from nclone_amd.vec_env import NppVecEnvironment

    env = NppVecEnvironment(_levels("mine"), N, level_ids=LEVEL_IDS, output=output, enable_state_stacking=True, state_stack_size=4,
                            frame_stack_padding_type="zero", checkpoint_slots=SLOTS)
    spawn = _copy_obs(env.reset(seed=0)[0])
    acts = _acts(31, 15).cpu().numpy()
    for t in range(10):
        obs = env.step(acts[t])[0]
    src_gs = _np(obs["game_state"])[3, -1].copy()
    st = env.archive_store(_slot_ids([(3, 5)]))
    assert _np(st).tolist() == [0 if e == 3 else 1 for e in range(N)]
    for t in range(10, 15):
        env.step(acts[t])
    slots = _slot_ids([(10, 5), (150, 5), (70, 5), (20, 6)])   # env 70 plays the other level, slot 6 is empty
    obs, info = env.reset(options={"checkpoint": {"slots": torch.from_numpy(slots).cuda() if output == "torch" else slots}})
    gs = _np(obs["game_state"])
    assert gs.shape == (N, 4, 41)
    for e in (10, 150):
        assert not gs[e, :3].any() and np.array_equal(gs[e, 3], src_gs), e
    for e in (20, 70, 0, 100):   # not restored: the spawn stack
        assert np.array_equal(gs[e], _np(spawn["game_state"])[e]), e
    restored = np.zeros(N, dtype=bool)
    restored[[10, 150]] = True
    status = np.where(slots < 0, 1, 0)
    status[70], status[20] = 2, 3
    assert info["checkpoint_replay"] is False
    assert np.array_equal(_np(info["restored"]), restored) and np.array_equal(_np(info["restore_status"]), status)
    with pytest.raises(NotImplementedError, match="frame stacking"):
        env.restart(slots)
    env.close()


@pytest.mark.parametrize("output", ["torch", "numpy"])
def test_vec_env_restart_between_steps(output):
    from nclone_amd.vec_env import NppVecEnvironment

    env = NppVecEnvironment(_reach_levels(), N, level_ids=LEVEL_IDS, output=output, enable_spatial_context=True,
                            enable_switch_states=True, enable_reachability=True, enable_visual_observations=True,
                            checkpoint_slots=SLOTS)
    env.reset(seed=0)
    acts = _acts(41, 12).cpu().numpy()
    for t in range(8):
        obs = env.step(acts[t])[0]
    src = _copy_obs(obs)
    env.archive_store(_slot_ids([(3, 5), (70, 0)]))
    for t in range(8, 12):
        obs, reward, *_ = env.step(acts[t])
    prev, prev_reward = _copy_obs(obs), _np(reward).copy()
    slots = _slot_ids([(10, 5), (150, 5), (100, 0), (20, 6), (75, 5)])   # slot 6 is empty, env 75 plays the other level
    got = env.restart(torch.from_numpy(slots).cuda() if output == "torch" else slots)
    assert set(got) == set(prev) and {"spatial_context", "switch_states", "reachability_features", "mine_sdf_features", "player_frame",
                                      "global_view", "game_state", "action_mask", "entity_positions"} <= set(got)
    moved = {10: 3, 150: 3, 100: 70}
    keep = np.array([e for e in range(N) if e not in moved])
    for k in got:
        g = _np(got[k])
        assert np.array_equal(g[keep], _np(prev[k])[keep]), k
        for dst, s in moved.items():
            assert np.array_equal(g[dst], _np(src[k])[s]), (k, dst)
    assert not np.array_equal(_np(got["game_state"])[10], _np(prev["game_state"])[10])
    assert np.array_equal(_np(env.batch.reward), prev_reward)   # the step's reward is left alone
    env.close()


def test_vec_env_restart_refuses_augmentation_and_serves_minimal_mode():
    from nclone_amd.vec_env import NppVecEnvironment

    env = NppVecEnvironment(_reach_levels(), 64, level_ids=np.zeros(64, dtype=np.int32), enable_visual_observations=True,
                            enable_augmentation=True, augmentation_seed=1, checkpoint_slots=2)
    with pytest.raises(NotImplementedError, match="frame augmentation"):
        env.restart(np.full(64, -1, dtype=np.int32))
    env.close()
    env = NppVecEnvironment(_reach_levels(), N, level_ids=LEVEL_IDS, observation_mode="minimal", checkpoint_slots=SLOTS)
    env.reset(seed=0)
    acts = _acts(51, 12).cpu().numpy()
    for t in range(8):
        obs = env.step(acts[t])[0]
    src = _copy_obs(obs)
    env.archive_store(_slot_ids([(3, 5)]))
    for t in range(8, 12):
        obs = env.step(acts[t])[0]
    prev = _copy_obs(obs)
    got = env.restart(_slot_ids([(10, 5), (150, 5)]))
    keep = np.array([e for e in range(N) if e not in (10, 150)])
    for k in got:
        assert np.array_equal(_np(got[k])[keep], _np(prev[k])[keep]), k
        for dst in (10, 150):
            assert np.array_equal(_np(got[k])[dst], _np(src[k])[3]), (k, dst)
    assert _np(got["minimal_observation"]).shape == (N, 40)
    env.close()


def test_single_env_adapter():
    from nclone_amd.vec_env import NppEnvironment

    env = NppEnvironment(map_data=_levels("mine")[0], checkpoint_slots=2)
    env.reset()
    for a in (2, 2, 5, 2, 2, 3):
        obs = env.step(a)[0]
    assert env.archive_store(1) == 0 and env.archive_store(2) == 4
    for a in (1, 1, 1):
        env.step(a)
    got, info = env.reset(options={"checkpoint": {"slots": [1]}})
    assert bool(info["restored"][0]) and np.array_equal(got["game_state"], obs["game_state"]) and got["player_x"] == obs["player_x"]
    env.close()


def test_scale_8192_permutation():
    n = 8192
    b = _batch(_levels("mine")[:1], n=n, level_ids=np.zeros(n, dtype=np.int32), slots=n)
    acts = _acts(61, 13, n)
    for t in range(8):
        b.step(acts[t])
    ids = torch.arange(n, dtype=torch.int32, device="cuda")
    st = b.archive_store(ids, ids, status=True)
    assert not st.any()
    f0, i0 = b.dump_state()
    for t in range(8, 13):
        b.step(acts[t])
    perm = np.random.default_rng(62).permutation(n).astype(np.int32)
    st = b.archive_restore(ids, torch.from_numpy(perm).cuda(), status=True)
    assert not st.any()
    f1, i1 = b.dump_state()
    assert len(np.unique(f0, axis=0)) > 64   # the stored states differ from env to env
    assert np.array_equal(f0[perm], f1) and np.array_equal(i0[perm], i1)
    b.close()
