"""GPU tests of the demonstration player (run with -m gpu on an MI355X; include/npp_amd.h npp_demo_create / npp_demo_play,
nclone_amd/demos.py) on the eight replays of tests/golden/demo.npz: the batched schedule against the
straightforward path (one env per replay through the existing tick / observe / reachability entries), against the rows the
reference's ReplayExecutor produced, the options, the refusals and the sampler."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

POS_TOL = 1e-5   # tests/test_gpu_parity.py: the north-star tolerance on float32 positions (its bar on traj.npz)
GS_TOL = 2e-6    # tests/test_gpu_parity.py: game_state f32 features (its bar on the reference's get_ninja_state rows)
ALL_KEYS = ("game_state", "action_mask", "entity_positions", "spatial_context", "reachability_features", "mine_sdf_features", "switch_states")
SENTINEL = 77    # no column and no row of any plane holds it: actions 0..5, flags < 8, done 0 / 1, game_state[3] = +-1 ...
ACTION_OF_BYTE = [0, 3, 2, 5, 1, 4, 0, 0]
_cache = {}


def _replays(golden):
    from nclone_amd.replay import CompactReplay

    z = golden.z("demo")
    return [CompactReplay(bytes(z["m%d" % r]), z["in%d" % r].tolist(), True, 1) for r in range(len(z["src"]))]


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def _played(golden, fs, n_envs, cap=10_000, action_mask="ones"):
    """One guarded play: {name: tensor [1 + rows + 1, dim]} pre-filled with the sentinel, plus the player's plan."""
    key = (fs, n_envs, cap, action_mask)
    if key not in _cache:
        from nclone_amd.demos import DemoPlayer

        p = DemoPlayer(_replays(golden), fs, cap, ALL_KEYS, n_envs, 0, action_mask)
        full = p.allocate(guard=1, fill=SENTINEL)
        p.play({k: v[1:-1] for k, v in full.items()})
        p.batch.sync()
        _cache[key] = (full, p.plan, p.level_ids.copy())
        p.close()
    return _cache[key]


def _straight(golden, fs):
    """The straightforward path: one env per replay, a dense input tensor, existing tick + observe + reachability per period, rows
    picked in torch.  -> ({name: [rows_total, dim]} in the dataset's order, env action-mask rows likewise)"""
    if ("straight", fs) in _cache:
        return _cache["straight", fs]
    from nclone_amd.engine import NppBatch

    reps = _replays(golden)
    n = len(reps)
    ids, levels, lid = {}, [], []
    for r in reps:
        if r.map_data not in ids:
            ids[r.map_data] = len(levels)
            levels.append(np.frombuffer(r.map_data, dtype=np.uint8))
        lid.append(ids[r.map_data])
    L = np.array([len(r.input_sequence) for r in reps])
    rows = L // fs
    b = NppBatch(n, autoreset=False, outputs=("spatial_context", "positions", "switch_states", "reachability_features", "mine_sdf_features",
                                              "reach_status"))
    b.load_levels(levels)
    b.assign_levels(np.array(lid))
    b.reset(mode="full")
    periods = int(rows.max())
    dense = np.zeros((periods * fs, n), dtype=np.uint8)
    for k, r in enumerate(reps):
        m = min(L[k], periods * fs)
        dense[:m, k] = r.input_sequence[:m]
    d_in = torch.from_numpy(dense).cuda()
    names = {"game_state": "game_state", "action_mask": "action_mask", "entity_positions": "entity_pos", "spatial_context": "spatial_context",
             "reachability_features": "reachability_features", "mine_sdf_features": "mine_sdf_features", "switch_states": "switch_states",
             "positions": "positions", "flags": "flags", "status": "reach_status"}
    per = {k: [] for k in names}
    for p in range(periods):
        b.tick(d_in[p * fs:(p + 1) * fs])
        b.observe()
        b.reachability(with_switch_states=True)
        for k, src in names.items():
            per[k].append(b.out.t[src].clone())
    b.sync()
    out = {}
    for k in names:
        st = torch.stack(per[k])   # [periods, n, ...]
        out[k] = torch.cat([st[:rows[r], r] for r in range(n)], 0)
    b.close()
    env_mask = out["action_mask"].clone()
    out["action_mask"] = torch.ones_like(env_mask)
    frame = np.concatenate([(np.arange(rows[r]) + 1) * fs - 1 for r in range(n)]).astype(np.int64)
    rep = np.concatenate([np.full(rows[r], r) for r in range(n)]).astype(np.int64)
    tv = np.array([max(0.0, (int(L[r]) - (int(f) + 1)) / int(L[r])) for r, f in zip(rep, frame)], dtype=np.float64).astype(np.float32)
    out["game_state"][:, 40] = torch.from_numpy(tv).cuda()
    out["flags"] = out["flags"] & 7
    out["frame"] = torch.from_numpy(frame.astype(np.int32)).cuda()
    out["replay"] = torch.from_numpy(rep.astype(np.int32)).cuda()
    out["level"] = torch.from_numpy(np.array(lid, dtype=np.int32)[rep]).cuda()
    out["action"] = torch.from_numpy(np.array([ACTION_OF_BYTE[reps[r].input_sequence[f]] for r, f in zip(rep, frame)], dtype=np.uint8)).cuda()
    done = np.zeros(len(rep), dtype=np.uint8)
    done[np.cumsum(rows)[rows > 0] - 1] = 1
    out["done"] = torch.from_numpy(done).cuda()
    _cache["straight", fs] = (out, env_mask, rows)
    return _cache["straight", fs]


@pytest.mark.parametrize("fs", [1, 4])
def test_schedules_agree_with_each_other_and_with_the_straight_path(golden, fs):
    """n_envs = 4: two rounds; n_envs = 8: one round.  At fs = 4 the 3-tick replay has no row, so seven replays are scheduled: an
    idle env in the second round of the one and in the only round of the other (at fs = 1 all eight play and no env idles).
    Every plane bit-identical between the two and with the straightforward path; guard rows untouched."""
    a, plan4, _ = _played(golden, fs, 4)
    b, plan8, _ = _played(golden, fs, 8)
    ref, _, rows = _straight(golden, fs)
    n_sched = int((rows > 0).sum())
    assert n_sched == (8 if fs == 1 else 7)
    assert len(plan4["round_ticks"]) == 2 and len(plan8["round_ticks"]) == 1
    assert np.array_equal(plan4["rows"], rows) and np.array_equal(plan8["rows"], rows)
    assert set(a) == set(b) == set(ref)
    total = int(rows.sum())
    for k in sorted(a):
        assert a[k].shape[0] == total + 2
        assert torch.equal(_bytes(a[k]), _bytes(b[k])), k
        assert torch.equal(_bytes(a[k][1:-1]), _bytes(ref[k])), (k, torch.nonzero((a[k][1:-1] != ref[k]).reshape(total, -1).any(1)).flatten()[:8])
        for g in (a[k][0], a[k][-1]):   # the guard rows still hold the sentinel
            assert bool((g == SENTINEL).all()), k
    # every row was written, a replay without rows contributes none, `done` closes every replay
    rep = a["replay"][1:-1].cpu().numpy()
    assert np.array_equal(np.bincount(rep, minlength=len(rows)), rows)
    if fs == 4:
        assert rows[7] == 0 and 7 not in rep
    done = a["done"][1:-1].cpu().numpy()
    last = np.cumsum(rows)[rows > 0] - 1
    assert done.sum() == len(last) and (done[last] == 1).all()
    assert bool((a["status"][1:-1] == 0).all())


@pytest.mark.parametrize("n_envs", [3, 5])
def test_idle_env_at_frame_skip_one(golden, n_envs):
    """fs = 1: all eight replays play, so 3 envs (three rounds, one idle env in the last) and 5 envs (two rounds, two idle) put
    an env without a replay through the feed and the collect kernel's early return at this frame skip as well."""
    a, plan, _ = _played(golden, 1, n_envs)
    ref, _, rows = _straight(golden, 1)
    assert len(plan["order"]) == 8 and len(plan["round_ticks"]) == -(-8 // n_envs) and 8 % n_envs != 0
    for k in sorted(a):
        assert torch.equal(_bytes(a[k][1:-1]), _bytes(ref[k])), k
        assert bool((a[k][0] == SENTINEL).all()) and bool((a[k][-1] == SENTINEL).all()), k


def test_level_the_reachability_tables_refuse(golden):
    """`005 toggley tutor` (reach3.npz: the level npp_reachability refuses, tests/test_reach_host.py): its transitions carry zero
    reachability rows, status 2 and valid False, alone and mixed with served levels in the caller's order; every other key
    equals a play without the reachability keys; served replays are untouched by the company."""
    from nclone_amd import _native as nat
    from nclone_amd.demos import DEFAULT_OBSERVATION_KEYS, DemoPlayer, load_demonstrations
    from nclone_amd.engine import reach_level_info
    from nclone_amd.replay import CompactReplay

    m = golden.z("reach3")["raised_m0"]
    assert not reach_level_info(m)["supported"]
    level = m.astype(np.uint8).tobytes()
    ra = CompactReplay(level, [2] * 9 + [3] * 4 + [0] * 6, True, 1)   # 19 ticks: 4 rows at fs = 4
    rb = CompactReplay(level, [4] * 8 + [5] * 5, True, 1)             # 13 ticks: 3 rows
    served = _replays(golden)
    reach = ("reachability_features", "mine_sdf_features")
    plain = tuple(k for k in DEFAULT_OBSERVATION_KEYS if k not in reach)
    cols = ("action", "frame", "done", "flags", "positions")

    with pytest.raises(nat.NppError) as e:   # the native object says so itself (and the player leaves no handle behind)
        DemoPlayer([ra], 4, 10_000, DEFAULT_OBSERVATION_KEYS, 2, 0, "ones")
    assert e.value.code == nat.NPP_ERR_UNSUPPORTED

    # (a) only the refused level, default keys
    alone = load_demonstrations([ra, rb], frame_skip=4, n_envs=2)
    bare = load_demonstrations([ra, rb], frame_skip=4, n_envs=2, observation_keys=plain)
    assert len(alone) == 7 and alone.rows.tolist() == [4, 3] and alone.replay.cpu().tolist() == [0] * 4 + [1] * 3
    assert set(alone.observations) == set(DEFAULT_OBSERVATION_KEYS)
    assert alone.observations["reachability_features"].shape == (7, 38) and alone.observations["mine_sdf_features"].shape == (7, 3)
    assert all(bool((alone.observations[k] == 0).all()) for k in reach)
    assert bool((alone.status == 2).all()) and not bool(alone.valid.any()) and bool((bare.status == 0).all())
    for k in plain:
        assert torch.equal(_bytes(alone.observations[k]), _bytes(bare.observations[k])), k
    for k in cols:
        assert torch.equal(_bytes(getattr(alone, k)), _bytes(getattr(bare, k))), k
    with pytest.raises(ValueError):
        alone.sample_batch(4)

    # (b) mixed with served levels, a failure in between: caller order kept
    failed = CompactReplay(served[1].map_data, served[1].input_sequence, False, 1)
    mixed = load_demonstrations([served[0], ra, failed, served[5], rb], frame_skip=4, n_envs=2)
    only = load_demonstrations([served[0], served[5]], frame_skip=4, n_envs=2)
    n0, n5 = len(served[0].input_sequence) // 4, len(served[5].input_sequence) // 4
    assert mixed.replay_index.tolist() == [0, 1, 3, 4] and mixed.rows.tolist() == [n0, 4, n5, 3]
    assert mixed.replay.cpu().tolist() == [0] * n0 + [1] * 4 + [3] * n5 + [4] * 3
    sl = mixed.episode_slices()
    is_refused = torch.zeros(len(mixed), dtype=torch.bool, device=mixed.status.device)
    is_refused[sl[1]] = True
    is_refused[sl[3]] = True
    assert torch.equal(mixed.status == 2, is_refused) and torch.equal(mixed.valid, ~is_refused)
    assert len(mixed.levels) == 3 and mixed.level.cpu()[[sl[0].start, sl[1].start, sl[2].start, sl[3].start]].tolist() == [0, 2, 1, 2]
    assert bytes(mixed.levels[2]) == level
    for k in DEFAULT_OBSERVATION_KEYS:
        got = mixed.observations[k]
        assert torch.equal(_bytes(torch.cat([got[sl[0]], got[sl[2]]])), _bytes(only.observations[k])), k
        want = bare.observations[k] if k in plain else torch.zeros_like(alone.observations[k])
        assert torch.equal(_bytes(torch.cat([got[sl[1]], got[sl[3]]])), _bytes(want)), k
    for k in cols:
        got = getattr(mixed, k)
        assert torch.equal(_bytes(torch.cat([got[sl[0]], got[sl[2]]])), _bytes(getattr(only, k))), k
        assert torch.equal(_bytes(torch.cat([got[sl[1]], got[sl[3]]])), _bytes(getattr(bare, k))), k
    idx = mixed.sample_batch(64, generator=torch.Generator().manual_seed(1))["indices"]
    assert bool(mixed.valid[idx].all())


@pytest.mark.parametrize("fs", [1, 4])
def test_rows_match_the_reference_executor(golden, fs):
    """Against demo.npz (ReplayExecutor.execute_replay's rows): action, frame, done and flags exact; game_state[0:40] and the
    positions within the bars the GPU parity tests apply to the reference's get_ninja_state and position fixtures; game_state[40]
    bit-equal."""
    z = golden.z("demo")
    planes, plan, _ = _played(golden, fs, 4)
    got = {k: planes[k][1:-1].cpu().numpy() for k in ("game_state", "positions", "action", "frame", "done", "flags", "replay")}
    worst_gs = worst_pos = 0.0
    at = 0
    for r in range(len(z["src"])):
        pre = "s%d_" % fs
        want = {k: z[pre + k + str(r)] for k in ("frame", "action", "gs", "pos", "flags")}
        n = len(want["frame"])
        assert plan["rows"][r] == n and plan["row_base"][r] == at
        s = slice(at, at + n)
        at += n
        assert (got["replay"][s] == r).all()
        assert np.array_equal(got["frame"][s], want["frame"]) and np.array_equal(got["action"][s], want["action"])
        assert np.array_equal(got["flags"][s], want["flags"]), (r, np.flatnonzero(got["flags"][s] != want["flags"]))
        assert np.array_equal(got["done"][s], (np.arange(n) == n - 1).astype(np.uint8))
        if n == 0:
            continue
        dg = np.abs(got["game_state"][s][:, :40] - want["gs"][:, :40]).max()
        dp = np.abs(got["positions"][s].astype(np.float32).astype(np.float64) - want["pos"].astype(np.float32).astype(np.float64)).max()
        worst_gs, worst_pos = max(worst_gs, dg), max(worst_pos, dp)
        print("fs %d replay %d rows %d: game_state diff %.3g, f32 position diff %.3g" % (fs, r, n, dg, dp))
        assert dg <= GS_TOL and dp <= POS_TOL, (r, dg, dp)
        assert np.array_equal(got["game_state"][s][:, 40].view(np.uint32), want["gs"][:, 40].view(np.uint32)), r
    assert at == got["frame"].shape[0]
    print("fs %d: worst game_state diff %.3g, worst f32 position diff %.3g" % (fs, worst_gs, worst_pos))


def test_options(golden):
    """The cap, the env's action mask, the success filter."""
    from nclone_amd.demos import load_demonstrations
    from nclone_amd.replay import CompactReplay

    full, plan, _ = _played(golden, 1, 4)
    capped, cplan, _ = _played(golden, 1, 4, cap=5)
    L = np.array([len(r.input_sequence) for r in _replays(golden)])
    assert np.array_equal(cplan["rows"], np.minimum(L, 5))
    first = np.concatenate([np.arange(b, b + min(n, 5)) for b, n in zip(plan["row_base"], plan["rows"])])
    idx = torch.from_numpy(first).cuda()
    for k in sorted(full):
        want = full[k][1:-1][idx]
        if k == "done":   # the cap moves the replay's last emitted row
            want = torch.from_numpy(np.concatenate([(np.arange(n) == n - 1) for n in cplan["rows"]]).astype(np.uint8)).cuda()
        assert torch.equal(_bytes(capped[k][1:-1]), _bytes(want)), k
        assert bool((capped[k][0] == SENTINEL).all()) and bool((capped[k][-1] == SENTINEL).all())
    env, _, _ = _played(golden, 4, 8, action_mask="env")
    ref, env_mask, _ = _straight(golden, 4)
    assert torch.equal(env["action_mask"][1:-1], env_mask) and not bool((env_mask == 1).all())
    for k in sorted(ref):
        if k != "action_mask":
            assert torch.equal(_bytes(env[k][1:-1]), _bytes(ref[k])), k
    # a failed replay (success byte 0) is skipped; paths and objects mix
    reps = _replays(golden)
    failed = CompactReplay(reps[1].map_data, reps[1].input_sequence, False, 1)
    ds = load_demonstrations([reps[0], failed, reps[5], CompactReplay.from_binary(reps[2].to_binary())], frame_skip=4, n_envs=2)
    assert ds.replay_index.tolist() == [0, 2, 3] and sorted(set(ds.replay.cpu().tolist())) == [0, 2, 3]
    assert len(ds) == sum(len(reps[i].input_sequence) // 4 for i in (0, 5, 2)) == int(ds.rows.sum())
    assert [s.stop - s.start for s in ds.episode_slices()] == ds.rows.tolist()
    assert set(ds.observations) == {"game_state", "reachability_features", "switch_states", "action_mask", "spatial_context", "mine_sdf_features"}
    assert bool(ds.valid.all()) and len(ds.levels) == 3 and ds.actions().dtype == torch.int64
    assert set(ds.to_numpy()) >= set(ds.observations) | {"action", "done", "frame", "replay", "level", "valid"}


def _create(b, inputs, levels, fs=1, cap=100, keys=1 | 128):
    inp = np.concatenate([np.asarray(i, dtype=np.uint8) for i in inputs])
    off = np.concatenate([[0], np.cumsum([len(i) for i in inputs])]).astype(np.int64)
    lv = np.asarray(levels, dtype=np.int32)
    return b.lib.npp_demo_create(b.h, inp.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p), lv.ctypes.data_as(C.c_void_p), len(inputs),
                                 fs, cap, keys)


def test_state_refusals_and_the_handle_afterwards(golden):
    from nclone_amd import _native as nat
    from nclone_amd.demos import DemoPlayer
    from nclone_amd.engine import NppBatch

    z = golden.z("demo")
    level = z["m5"]   # the door level (corpus 127)
    inputs = [z["in5"][:12], z["in5"][:7]]
    b = NppBatch(4, autoreset=True)
    b.load_levels([level])
    assert _create(b, inputs, [0, 0]) == nat.NPP_OK
    for on, off in ((lambda: b.set_routes(16), lambda: b.set_routes(0)),
                    (lambda: b.set_reward_mode("pbrs"), lambda: b.set_reward_mode("sparse")),
                    (lambda: b.set_action_masking("hard"), lambda: b.set_action_masking(None)),
                    (lambda: b.set_frame_stack(0, 2), lambda: b.set_frame_stack(0, 0)),
                    (lambda: b.set_level_pool([1.0]), lambda: b.set_level_pool(None))):
        on()
        assert _create(b, inputs, [0, 0]) == nat.NPP_ERR_STATE
        off()
        assert _create(b, inputs, [0, 0]) == nat.NPP_OK
    assert _create(b, inputs, [0, 1]) == nat.NPP_ERR_INVALID and _create(b, inputs, [-1, 0]) == nat.NPP_ERR_INVALID
    assert _create(b, inputs, [0, 0], fs=0) == nat.NPP_ERR_INVALID
    total = C.c_int64(-1)
    assert b.lib.npp_demo_rows(b.h, C.byref(total), None, None) == nat.NPP_OK and total.value == 19
    b.load_levels([level])   # a new level set drops the object
    assert b.lib.npp_demo_rows(b.h, C.byref(total), None, None) == nat.NPP_ERR_STATE
    assert b.lib.npp_demo_play(b.h, C.byref(nat.DemoOut())) == nat.NPP_ERR_STATE
    b.close()

    # a short step run after a play gives the bits of a fresh handle
    reps = _replays(golden)[3:6]
    p = DemoPlayer(reps, 4, 10_000, ALL_KEYS, 4, 0, "ones")
    planes = p.allocate()
    p.play(planes)
    lv = np.array([0, 1, 2, 1], dtype=np.int32)
    acts = torch.from_numpy(np.random.default_rng(3).integers(0, 6, size=(12, 4)).astype(np.uint8)).cuda()

    def run(batch):
        batch.assign_levels(lv)
        rows = []
        for s in range(len(acts)):
            batch.step(acts[s], frame_skip=4)
            rows.append(torch.cat([_bytes(batch.game_state).flatten(), batch.flags.flatten(), _bytes(batch.action_mask).flatten()]).clone())
        batch.sync()
        return torch.stack(rows), batch.dump_state()

    got, (gf, gi) = run(p.batch)
    fresh = NppBatch(4, autoreset=False)
    fresh.load_levels(p.levels)
    want, (wf, wi) = run(fresh)
    assert torch.equal(got, want) and np.array_equal(gf, wf) and np.array_equal(gi, wi)
    p.close()
    fresh.close()


def test_sample_batch_returns_the_rows_of_its_indices(golden):
    from nclone_amd.demos import load_demonstrations

    ds = load_demonstrations(_replays(golden), frame_skip=4, observation_keys=ALL_KEYS, n_envs=4)
    g = torch.Generator().manual_seed(5)
    batch = ds.sample_batch(64, generator=g)
    idx = batch["indices"]
    assert idx.shape == (64,) and int(idx.min()) >= 0 and int(idx.max()) < len(ds) and len(set(idx.cpu().tolist())) > 16
    assert set(batch["observations"]) == set(ALL_KEYS)
    for k, v in batch["observations"].items():
        assert torch.equal(_bytes(v), _bytes(ds.observations[k][idx])), k
    assert batch["actions"].dtype == torch.int64 and torch.equal(batch["actions"], ds.action[idx].long())
    again = ds.sample_batch(64, generator=torch.Generator().manual_seed(5))
    assert torch.equal(again["indices"], idx)
    assert not torch.equal(ds.sample_batch(64, generator=g)["indices"], idx)
