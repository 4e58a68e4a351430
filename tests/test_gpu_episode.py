"""GPU tests of the episode statistics (include/npp_amd.h npp_set_episode_stats, nclone_amd/csrc/npp_episode.hpp / npp_episode.hip;
DESIGN.md 24).  The device is held against the Python model of the rule (tests/episode_ref.py), which is fed the flags, frames and
reward rows the batch reports: planes, table and the `ended` row must be equal bit for bit.  The absolute check plays the
reference's recorded rollouts (tests/golden/reward.npz) and compares each finished episode with the fixture's own sums."""
import os

import numpy as np
import pytest

from tests import episode_ref as ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


def _fix():
    if "fix" not in _cache:
        z = np.load(os.path.join(ROOT, "tests", "golden", "reward.npz"))
        names = bytes(z["names"]).decode().split("\n")
        _cache["fix"] = (z, names)
    return _cache["fix"]


def _three_levels():
    """a level the recorded actions win (doors), one they die on (mines), and one no env plays"""
    z, names = _fix()
    ks = [names.index("doors:replay:127"), names.index("mines:replay:24"), names.index("c0:replay:0")]
    return z, ks, [z["m%d" % k] for k in ks]


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _batch(levels, n, level_ids, autoreset=True, trunc=100000, outputs=(), stats=True, **kw):
    from nclone_amd.engine import NppBatch

    b = NppBatch(n, autoreset=autoreset, outputs=outputs, fast_reset=False, **kw)
    b.load_levels(levels)
    b.assign_levels(np.asarray(level_ids, dtype=np.int32))
    b.set_truncation_limit(trunc)
    if stats:
        b.set_episode_stats(True)
    b.reset()
    return b


def _device(b):
    v = b.episode_views()
    b.sync()
    return v["i32"].cpu().numpy(), v["f64"].cpu().numpy(), v["table"].cpu().numpy()


def _check(b, m, what=""):
    i32, f64, table = _device(b)
    wi, wd = m.planes()
    bad = np.argwhere(i32 != wi)
    assert len(bad) == 0, (what, bad[:5], i32[:, bad[0][1]], wi[:, bad[0][1]])
    bad = np.argwhere(f64.view(np.uint64) != wd.view(np.uint64))
    assert len(bad) == 0, (what, bad[:5])
    assert np.array_equal(table, m.table_i64()), (what, table, m.table_i64())
    return i32, f64, table


class Run:
    """a batch and its model, stepped together"""

    def __init__(self, b, n_levels, level_ids, autoreset=True):
        self.b, self.m = b, ref.Model(b.n, n_levels, autoreset)
        self.levels = np.asarray(level_ids, dtype=np.int32)
        self.ended = torch.zeros(b.n, dtype=torch.uint8, device="cuda")
        self.flags_seen = 0
        self.m.event(ref.EV_RESET, self.levels)   # _batch's reset, after the INIT

    def step(self, act, skip=4, pool=False, what=""):
        b = self.b
        b.step(act, frame_skip=skip)
        b.episode_accumulate(ended=self.ended)
        b.sync()
        flags, frames, reward = b.flags.cpu().numpy(), b.frames.cpu().numpy(), b.reward.cpu().numpy()
        if pool:
            self.levels = b.env_levels()
        want = self.m.accumulate(flags, frames.astype(np.uint16), reward, self.levels)
        got = self.ended.cpu().numpy()
        assert np.array_equal(got, want), (what, np.flatnonzero(got != want)[:5])
        self.flags_seen |= int(np.bitwise_or.reduce(flags[got != 0])) if got.any() else 0
        return flags, got

    def reset(self, mask):
        self.b.reset(mask)
        self.m.event(ref.EV_RESET, self.levels, mask)


def _mixed_actions(z, ks, level_ids, n, steps, seed):
    """random actions, except that the first eight envs follow the recorded actions of their level"""
    act = np.random.default_rng(seed).integers(0, 6, size=(steps, n)).astype(np.uint8)
    for e in range(8):
        a = z["aact%d" % ks[level_ids[e]]][:steps]
        act[:len(a), e] = a
    return _cuda(act)


def test_mixed_rollout_with_autoreset():
    """67 envs (a partial wavefront) on two of three loaded levels, 200 steps at frame skip 4, truncation after 400 frames: every
    step's planes-relevant rows go through the model; all three endings occur."""
    z, ks, levels = _three_levels()
    n = 67
    ids = np.arange(n) % 2
    b = _batch(levels, n, ids, trunc=400)
    r = Run(b, 3, ids)
    act = _mixed_actions(z, ks, ids, n, 200, 1)
    for t in range(200):
        r.step(act[t], what=t)
        if t % 40 == 39:
            _check(b, r.m, t)
    i32, f64, table = _check(b, r.m, "end")
    assert r.flags_seen & 11 == 11, r.flags_seen   # won, dead and truncated episodes ended
    assert table[2].sum() == 0 and (table[:2, ref.COL["episodes"]] > 0).all() and table[:, ref.COL["abandoned"]].sum() == 0
    assert table[0, ref.COL["won"]] > 0 and table[1, ref.COL["dead"]] > 0 and table[:, ref.COL["truncated"]].sum() > 0
    assert table[:, ref.COL["episodes"]].sum() == int(i32[ref.N_FINISHED].sum())
    assert not (i32[ref.BITS] & ref.CLOSED).any()
    b.close()


def test_mixed_rollout_without_autoreset_and_masked_resets():
    """the same without auto-reset: ended envs close, truncated ones keep stepping and are not counted again; every 25 steps the
    closed envs and a few running ones are reset (`abandoned`)."""
    z, ks, levels = _three_levels()
    n = 67
    ids = np.arange(n) % 2
    b = _batch(levels, n, ids, autoreset=False, trunc=200)
    r = Run(b, 3, ids, autoreset=False)
    act = _mixed_actions(z, ks, ids, n, 200, 2)
    closed_rows = 0
    for t in range(200):
        was_closed = np.array([bool(q.i[ref.BITS] & ref.CLOSED) for q in r.m.rec])
        flags, _ = r.step(act[t], what=t)
        frames = b.frames.cpu().numpy()
        closed_rows += int((was_closed & (frames > 0)).sum())   # a truncated env stepped on
        if t % 25 == 24:
            mask = was_closed.astype(np.uint8)
            mask[t % n] = mask[(t + 7) % n] = 1
            _check(b, r.m, ("before reset", t))
            r.reset(mask)
            _check(b, r.m, ("after reset", t))
    i32, f64, table = _check(b, r.m, "end")
    assert closed_rows > 0 and table[:, ref.COL["abandoned"]].sum() > 0 and r.flags_seen & 11 == 11, (closed_rows, r.flags_seen)
    assert table[:, ref.COL["episodes"]].sum() == int(i32[ref.N_FINISHED].sum())
    b.close()


def test_absolute_against_the_reference_fixture():
    """reward_mode="pbrs" along rollouts "a" (frame skip 4) and "b" (frame skip 1) of reward.npz, one env per level: at each of
    the fixture's episode ends the finished steps and frames equal the fixture's sums exactly, and ret, comp[0] (pbrs) and comp[4]
    (terminal) equal its f64 sums within sum |v_i| * 2^-24 -- the f32 rounding of each summand, nothing else."""
    z, names = _fix()
    ok = [k for k in range(len(names)) if not np.isinf(z["const%d" % k]).any()]
    n = len(ok)
    b = _batch([z["m%d" % k] for k in ok], n, np.arange(n), outputs=("positions", "reward_components"))
    b.observe()
    b.set_reward_mode("pbrs")
    ended = torch.zeros(n, dtype=torch.uint8, device="cuda")
    checked = 0
    for phase, skip in (("a", 4), ("b", 1)):
        steps = max(len(z["%sact%d" % (phase, k)]) for k in ok)
        act = np.zeros((steps, n), dtype=np.uint8)
        for e, k in enumerate(ok):
            a = z["%sact%d" % (phase, k)]
            act[:len(a), e] = a
        if phase == "b":
            b.reset(mode="full")
            b.observe()
        act = _cuda(act)
        start = [0] * n
        for t in range(steps):
            b.step(act[t], frame_skip=skip)
            b.step_reward()
            b.episode_accumulate(components=b.out.t["reward_components"], ended=ended)
            b.sync()
            got = ended.cpu().numpy()
            if not got.any():
                continue
            i32, f64, _ = _device(b)
            for e, k in enumerate(ok):
                m = len(z["%sact%d" % (phase, k)])
                if t >= m:
                    continue
                assert bool(got[e]) == bool(z["%sflags%d" % (phase, k)][t] & 3), (phase, names[k], t)
                if not got[e]:
                    continue
                s = slice(start[e], t + 1)
                assert i32[ref.FIN + ref.STEPS, e] == t + 1 - start[e], (phase, names[k], t)
                assert i32[ref.FIN + ref.FRAMES, e] == int(z["%sframes%d" % (phase, k)][s].astype(np.int64).sum()), (phase, names[k], t)
                for plane, v in ((ref.DFIN + ref.RET, z["%srew%d" % (phase, k)][s]),
                                 (ref.DFIN + ref.COMP + 0, z["%scomp%d" % (phase, k)][s, 0]),
                                 (ref.DFIN + ref.COMP + 4, z["%scomp%d" % (phase, k)][s, 3])):   # (the fixture's fourth column: terminal)
                    want = 0.0
                    for x in v:
                        want += float(x)
                    bound = float(np.abs(v).sum()) * 2.0 ** -24
                    print("%s %s t=%d plane %d: device %.17g fixture %.17g bound %.3g" % (phase, names[k], t, plane, f64[plane, e], want, bound))
                    assert abs(f64[plane, e] - want) <= bound, (phase, names[k], t, plane, f64[plane, e], want, bound)
                start[e] = t + 1
                checked += 1
    assert checked >= 30, checked
    b.close()


@pytest.mark.parametrize("n", [256, 320])
def test_contention_every_env_ends_on_the_same_rows(golden, n):
    """one block, then two, all on one level and one plan of routes.npz: every env ends on the same rows, so each ending row sends
    n episodes to one table row at once.  The table must be n times one env's."""
    r = golden.z("routes")
    k = golden.names("routes").index("mines:hcorr:mines:100001")
    plan, marks = r["a%d" % k][:120], r["t%d" % k][:120]
    b = _batch([r["m%d" % k]], n, np.zeros(n))
    one = ref.Model(1, 1, True)
    one.event(ref.EV_RESET, [0])
    d_plan = _cuda(np.repeat(plan[:, None], n, axis=1))
    ended = torch.zeros(n, dtype=torch.uint8, device="cuda")
    for s in range(len(plan)):
        b.step(d_plan[s], 4)
        b.episode_accumulate(ended=ended)
        b.sync()
        flags, frames, reward = b.flags.cpu().numpy(), b.frames.cpu().numpy(), b.reward.cpu().numpy()
        assert (flags == flags[0]).all() and (frames == frames[0]).all() and (reward.view(np.uint32) == reward.view(np.uint32)[0]).all(), s
        e = one.accumulate(flags[:1], frames[:1].astype(np.uint16), reward[:1], [0])
        assert bool(e[0]) == bool(marks[s]) and (ended.cpu().numpy() == e[0]).all(), s
    i32, f64, table = _device(b)
    t1 = one.table[0]
    assert t1[ref.COL["episodes"]] == int(marks.sum()) >= 10
    assert [int(v) & ref.M64 for v in table[0].view(np.uint64)] == [(n * v) & ref.M64 for v in t1], (table[0], t1)
    wi, wd = one.planes()
    assert (i32 == wi).all() and (f64.view(np.uint64) == wd.view(np.uint64)).all()
    b.close()


def test_level_pool_charges_the_level_played():
    """level pool on, two levels: npp_step has drawn the next level when the ending row is accumulated; the episode is charged to
    the level it was played on and the new one starts on the drawn level."""
    z, ks, levels = _three_levels()
    n = 67
    ids = np.arange(n) % 2
    b = _batch(levels[:2], n, ids, trunc=120)
    b.set_level_pool([1.0, 2.0], seed=5)
    r = Run(b, 2, ids)
    act = _cuda(np.random.default_rng(3).integers(0, 6, size=(100, n)).astype(np.uint8))
    moved = 0
    for t in range(100):
        before = r.levels.copy()
        _, got = r.step(act[t], pool=True, what=t)
        moved += int(((before != r.levels) & (got != 0)).sum())
        assert ((before == r.levels) | (got != 0)).all()   # only ended envs changed level
    i32, f64, table = _check(b, r.m, "end")
    assert moved > 10 and (table[:, ref.COL["episodes"]] > 0).all()
    fin = i32[ref.N_FINISHED] > 0
    assert (i32[ref.LEVEL][fin] == r.levels[fin]).all()
    # npp_draw_levels: the envs that changed level restart, a running episode counts as abandoned
    r.step(act[0], pool=True)
    before = r.levels.copy()
    b.draw_levels()
    r.levels = b.env_levels()
    changed = (before != r.levels).astype(np.uint8)
    assert changed.any() and not changed.all()
    r.m.event(ref.EV_RESET, r.levels, changed)
    _, _, table = _check(b, r.m, "draw_levels")
    assert table[:, ref.COL["abandoned"]].sum() > 0
    b.close()


def test_events():
    """archive restore and snapshot restore (`restored` only), npp_tick, npp_assign_levels, npp_load_levels switches the feature
    off, the entries are NPP_ERR_STATE while off"""
    from nclone_amd import _native as nat
    from nclone_amd._native import NppError

    z, ks, levels = _three_levels()
    n = 67
    ids = np.arange(n) % 2
    b = _batch(levels, n, ids, trunc=240, stats=False)
    for call in (b.episode_views, b.episode_accumulate, b.episode_restart, b.episode_table_reset):
        with pytest.raises(NppError) as ei:
            call()
        assert ei.value.code == nat.NPP_ERR_STATE and "npp_set_episode_stats" in str(ei.value)
    b.set_episode_stats(True)
    b.archive_create(8)
    r = Run(b, 3, ids)
    r.m.event(ref.EV_INIT, ids)   # (no reset since the feature was switched on)
    _check(b, r.m, "init")
    act = _mixed_actions(z, ks, ids, n, 90, 4)
    for t in range(20):
        r.step(act[t])
    # snapshot + archive store, more steps, then restores
    b.snapshot()
    assert b.archive_store([3, 4], [0, 1], status=True).cpu().numpy().tolist() == [0, 0]
    for t in range(20, 30):
        r.step(act[t])
    envs, slots = np.array([3, 4, 5, 6], dtype=np.int32), np.array([0, 1, 2, 0], dtype=np.int32)   # slot 2 is empty, slot 0 holds level 1
    status = b.archive_restore(envs, slots, status=True).cpu().numpy()
    assert status[0] == 0 and status[1] == 0 and status[2] != 0 and status[3] != 0, status
    mask = np.zeros(n, dtype=np.uint8)
    mask[envs[status == 0]] = 1
    r.m.event(ref.EV_RESTORE, ids, mask)
    _check(b, r.m, "archive restore with status")
    b.archive_restore(np.array([8, 7], dtype=np.int32), np.array([1, 2], dtype=np.int32))   # the caller asks for no status; slot 2 is empty
    mask[:] = 0
    mask[8] = 1
    r.m.event(ref.EV_RESTORE, ids, mask)
    _check(b, r.m, "archive restore without status")
    mask[:] = 0
    mask[10:20] = 1
    b.restore(mask)
    r.m.event(ref.EV_RESTORE, ids, mask)
    i32, _, table = _check(b, r.m, "snapshot restore")
    assert (i32[ref.BITS][[3, 4, 8] + list(range(10, 20))] == ref.FROM_RESTORE).all() and table[:, ref.COL["abandoned"]].sum() > 0
    before = table.copy()
    for t in range(30, 90):
        r.step(act[t])
    i32, _, table = _check(b, r.m, "after the restored episodes ended")
    d = table - before
    assert d[:, ref.COL["restored"]].sum() >= 5 and d[:, ref.COL["episodes"]].sum() > 0
    # raw ticks mark the current episodes
    b.tick(_cuda(np.zeros((3, n), dtype=np.uint8)))
    r.m.event(ref.EV_TICK, ids)
    i32, _, _ = _check(b, r.m, "tick")
    assert (i32[ref.BITS] & ref.TICKED).all()
    # explicit restart through the C entry, with a device mask
    mask[:] = 0
    mask[::3] = 1
    b.episode_restart(_cuda(mask), from_restore=True)
    r.m.event(ref.EV_RESTORE, ids, mask)
    _check(b, r.m, "episode_restart")
    # a new assignment of some envs: RESET on the new level
    new = ids.copy()
    new[:5] = 2
    b.assign_levels(new[:5], env_ids=np.arange(5))
    mask[:] = 0
    mask[:5] = 1
    r.levels = new
    r.m.event(ref.EV_RESET, new, mask)
    i32, _, _ = _check(b, r.m, "assign_levels")
    assert (i32[ref.LEVEL][:5] == 2).all()
    for t in range(5):
        r.step(act[t])
    _check(b, r.m, "on the new level")
    b.episode_table_reset()
    r.m.table = ref.new_table(3)
    _check(b, r.m, "table reset")
    # a new level set switches the feature off
    b.load_levels(levels[:2])
    with pytest.raises(NppError) as ei:
        b.episode_views()
    assert ei.value.code == nat.NPP_ERR_STATE
    b.set_episode_stats(True)
    assert b.episode_level_table().shape == (2, 16)
    b.close()


def test_seeding_clears_the_current_records_without_counting():
    from tests import seed_ref as sref

    from nclone_amd.vec_env import NppVecEnvironment

    reps = sref.Replays(sref.fixture())
    env = NppVecEnvironment(reps.levels, 3, level_ids=np.arange(3) % len(reps.levels), frame_skip=1, truncation_limit=10000, checkpoint_slots=64,
                            checkpoint_cells=True, episode_stats=True)
    env.reset()
    for _ in range(5):
        env.step(np.zeros(3, dtype=np.uint8))
    b = env.batch
    i32, _, before = _device(b)
    assert (i32[ref.STEPS] == 5).all()
    env.seed_archive_from_replays(reps.compact())
    i32, f64, table = _device(b)
    assert not i32[:ref.LEVEL].any() and not i32[ref.BITS].any() and not f64[:ref.DFIN].any()
    assert np.array_equal(table, before)
    env.close()


@pytest.mark.parametrize("which", ["mine", "door"])
def test_step_many_equals_single_steps(which):
    from nclone_amd import levels as lv

    levels = getattr(lv, which + "_levels")()[0][:2]
    n = 67
    ids = np.arange(n) % 2
    act = _cuda(np.random.default_rng(6).integers(0, 6, size=(24, n)).astype(np.uint8))
    out = []
    for many in (False, True):
        b = _batch(levels, n, ids, trunc=60)
        for c in range(3):
            if many:
                flags, reward, frames = b.step_many(act[8 * c:8 * c + 8])
                b.episode_accumulate(flags, frames, reward, n_steps=8)
            else:
                for t in range(8 * c, 8 * c + 8):
                    b.step(act[t])
                    b.episode_accumulate()
        out.append(_device(b))
        b.close()
    for x, y in zip(*out):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert out[0][2][:, ref.COL["episodes"]].sum() > 0


def test_obs_overlap_same_bits():
    from nclone_amd import levels as lv

    levels = lv.door_levels()[0][:2]
    n = 192
    ids = (np.arange(n) // 64) % 2
    act = _cuda(np.random.default_rng(8).integers(0, 6, size=(60, n)).astype(np.uint8))
    out = []
    for overlap in (0, 40):
        b = _batch(levels, n, ids, trunc=100)
        if overlap:
            b.set_obs_overlap(overlap)
        for t in range(60):
            b.step(act[t])
            b.episode_accumulate()
        out.append(_device(b))
        b.close()
    for x, y in zip(*out):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert out[0][2][:, ref.COL["episodes"]].sum() > 0


def _np(v):
    return v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


@pytest.mark.parametrize("output", ["torch", "numpy"])
def test_vec_env_info(output):
    """info["_episode"] / info["episode"] in both output modes, in pbrs mode: the mask is the step's done, the rows are the model's
    finished episodes, rows outside the mask keep the previous one; episode_level_stats(); the checkpoint reset marks from_checkpoint."""
    from nclone_amd.vec_env import NppVecEnvironment

    z, ks, levels = _three_levels()
    n = 8
    ids = np.arange(n) % 2
    env = NppVecEnvironment(levels[:2], n, level_ids=ids, truncation_limit=400, fast_reset=False, output=output, reward_mode="pbrs",
                            episode_stats=True)
    env.reset()
    m = ref.Model(n, 2, True)
    m.event(ref.EV_RESET, ids)
    act = _mixed_actions(z, ks, ids, n, 110, 9).cpu().numpy()
    last = None
    for t in range(110):
        _obs, rew, term, trunc, info = env.step(act[t])
        b = env.batch
        b.sync()
        comps = b.out.t["reward_components"].cpu().numpy()
        ended = m.accumulate(b.flags.cpu().numpy(), b.frames.cpu().numpy().astype(np.uint16), b.reward.cpu().numpy(), ids, comps[None])
        done = _np(term) | _np(trunc)
        assert np.array_equal(_np(info["_episode"]), done) and np.array_equal(done, ended != 0), t
        ep = {k: _np(v).copy() for k, v in info["episode"].items()}
        assert set(ep) == {"r", "l", "steps", "is_success", "switch_activated", "switch_activation_frame", "level_id", "from_checkpoint",
                           "pbrs_total", "terminal_reward"}
        wi, wd = m.planes()
        assert np.array_equal(ep["r"].view(np.uint64), wd[ref.DFIN + ref.RET].view(np.uint64)), t
        assert np.array_equal(ep["pbrs_total"].view(np.uint64), wd[ref.DFIN + ref.COMP].view(np.uint64)), t
        assert np.array_equal(ep["terminal_reward"].view(np.uint64), wd[ref.DFIN + ref.COMP + 4].view(np.uint64)), t
        assert np.array_equal(ep["l"], wi[ref.FIN + ref.FRAMES]) and np.array_equal(ep["steps"], wi[ref.FIN + ref.STEPS]), t
        assert np.array_equal(ep["is_success"], (wi[ref.FIN_FLAGS] & 1) != 0) and np.array_equal(ep["level_id"], wi[ref.FIN + ref.LEVEL]), t
        sw = wi[ref.FIN + ref.SWITCH_STEP] != 0
        assert np.array_equal(ep["switch_activated"], sw), t
        assert np.array_equal(ep["switch_activation_frame"], np.where(sw, wi[ref.FIN + ref.SWITCH_FRAMES], -1)), t
        assert not ep["from_checkpoint"].any()
        if last is not None:
            for k in ep:   # rows outside the mask hold the previous finished episode
                assert np.array_equal(ep[k][~done], last[k][~done]), (t, k)
        last = ep
    assert last["is_success"].any() and (last["steps"] > 0).all()
    st = {k: _np(v) for k, v in env.episode_level_stats().items()}
    table = m.table_i64()
    for k, name in enumerate(ref.COLUMNS):
        assert np.array_equal(st[name], table[:, k]), name
    assert np.array_equal(st["success_rate"], table[:, 1] / table[:, 0])
    assert np.allclose(st["mean_return"], [ref.fix_to_float(table[q, ref.COL["return_fix"]]) / table[q, 0] for q in range(2)], rtol=1e-15, atol=0)
    env.reset_episode_level_stats()
    st = {k: _np(v) for k, v in env.episode_level_stats().items()}
    assert not any(v.any() for v in st.values())   # rates are 0 where a level has no episode
    # a checkpoint replay: its steps are not accumulated, and the episode that follows is marked
    env.reset(options={"checkpoint": act[:5, 0]})
    i32, _, table = _device(env.batch)
    assert (i32[ref.BITS] == ref.FROM_RESTORE).all() and not i32[ref.STEPS].any()
    assert not np.delete(table, ref.COL["abandoned"], axis=1).any()   # (the reset abandoned the running episodes)
    seen = np.zeros(n, dtype=bool)
    for t in range(110):
        _obs, rew, term, trunc, info = env.step(act[t])
        e, fc = _np(info["_episode"]), _np(info["episode"]["from_checkpoint"])
        assert fc[e & ~seen].all() and not fc[e & seen].any(), t   # an env's first episode after the replay, and only that one
        seen |= e
        if seen.all():
            break
    assert seen.all()
    st = {k: _np(v) for k, v in env.episode_level_stats().items()}
    assert st["restored"].sum() == n
    env.close()


def test_single_env_keys_and_async_refusal():
    from nclone_amd.async_env import NppAsyncVecEnvironment
    from nclone_amd.vec_env import NppEnvironment

    z, names = _fix()
    k = names.index("c0:replay:0")
    env = NppEnvironment(map_data=z["m%d" % k], truncation_limit=100000, fast_reset=False, episode_stats=True)
    env.reset()
    ret, frames = 0.0, 0
    for t in range(40):
        _obs, rew, term, trunc, info = env.step(int(z["aact%d" % k][t]))
        ret += float(np.float32(rew))
        frames += info["frame_skip_stats"]["frames_executed"]
        if term or trunc:
            assert info["r"] == ret and info["l"] == frames and info["is_success"] is True and 0 < info["switch_activation_frame"] <= frames
            break
        assert "r" not in info and "l" not in info
    else:
        raise AssertionError("the recorded episode did not end")
    assert t == int(np.flatnonzero(z["aflags%d" % k] & 3)[0])
    env.close()
    with pytest.raises(ValueError, match="episode_stats"):
        NppAsyncVecEnvironment([z["m%d" % k]], 8, n_streams=2, episode_stats=True)
