"""GPU tests of the action routes (include/npp_amd.h npp_set_routes, nclone_amd/csrc/npp_route.hpp / npp_route.hip):
the device keeps, per env, the list of actions the reference's env keeps (tests/golden/routes.npz, made by running the reference);
a route replayed from the spawn reproduces the state it was stored with, bit for bit; archive records carry routes and a restore
puts a slot's route into the env; won episodes survive the auto-reset; the bits; one rule on every path (single steps, step_many,
the observation overlap, a caller without flags / frames rows); every reset flips; the cell index's slots replay; layout and
refusals; the host classes.  Wherever flags and frames are at hand the device is also held against the Python model of the rule
(tests/route_ref.py).  The base shape is tests/test_gpu_archive.py's: 192 envs, blocks 0 and 2 on level 0, block 1 on level 1."""
import ctypes as C

import numpy as np
import pytest

from tests import route_ref as ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, SLOTS, CAP = 192, 8, 64
LEVEL_IDS = (np.arange(N) // 64) % 2
SRC_ENVS, SRC_SLOTS = [3, 70, 130], [5, 0, 2]            # stored: level 0, level 1, level 0
POS_TOL = 1e-5   # tests/test_gpu_parity.py: the north-star tolerance on float32 positions
EMPTY_HDR = ref.EMPTY + ref.EMPTY + [0, 0, 0, 0]


def _levels(which):
    from nclone_amd import levels as lv

    return getattr(lv, which + "_levels")()[0][:2]


def _batch(levels, cap=CAP, autoreset=True, n=N, level_ids=LEVEL_IDS, slots=SLOTS, outputs=()):
    from nclone_amd.engine import NppBatch

    b = NppBatch(n, autoreset=autoreset, outputs=outputs)
    b.load_levels(levels)
    b.assign_levels(level_ids)
    if cap:
        b.set_routes(cap)
    if slots:
        b.archive_create(slots)
    return b


def _acts(seed, steps, n=N):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 6, size=(steps, n)).astype(np.uint8)).cuda()


def _routes(b):
    """(header i32 [n, 16], actions u8 [n, 2, cap]) on the host."""
    act, hdr = b.route_views()
    b.sync()
    return hdr.cpu().numpy(), act.cpu().numpy()


def _cur(h, a, e):
    return a[e, h[e, 12], :h[e, 0]]


def _fin(h, a, e):
    return a[e, 1 - h[e, 12], :h[e, 6]]


def _full(b, envs):
    f, i = b.dump_state()
    cs = b.entity_checksum()
    return {"f": f, "i": i, "cs": cs, "ent": {int(e): b.dump_entities(int(e)) for e in envs}}


def _rows_equal(a, ea, b, eb):
    return (np.array_equal(a["f"][ea], b["f"][eb]) and np.array_equal(a["i"][ea], b["i"][eb]) and
            np.array_equal(a["cs"][ea], b["cs"][eb], equal_nan=True) and np.array_equal(a["ent"][ea], b["ent"][eb]))


class Model:
    """tests/route_ref.py for every env of a batch, fed with what the batch reports."""

    def __init__(self, b, cap, autoreset=True):
        self.b, self.r = b, [ref.Route(cap, autoreset) for _ in range(b.n)]

    def step(self, acts_row, fs, levels=None):
        """after b.step(acts_row, fs): the step's flags and frames rows"""
        self.b.sync()
        flags, frames = self.b.flags.cpu().numpy(), self.b.frames.cpu().numpy()
        levels = LEVEL_IDS if levels is None else levels
        a = acts_row.cpu().numpy()
        for e, r in enumerate(self.r):
            r.step(int(a[e]), int(flags[e]), int(frames[e]), fs, int(levels[e]))
        return flags, frames

    def check(self, what=""):
        h, a = _routes(self.b)
        for e, r in enumerate(self.r):
            assert h[e].tolist() == r.hdr, (what, e, h[e].tolist(), r.hdr)
            assert np.array_equal(_cur(h, a, e), r.current()), (what, e)
            assert np.array_equal(_fin(h, a, e), r.finished()), (what, e)
        return h, a


@pytest.mark.parametrize("k", range(5))
def test_reference_episodes(golden, k):
    """The fixture's plan on 64 envs with auto-reset (Simulator.reset): at every checkpoint step the current route is the
    reference's action_sequence, after every terminal step the finished route is the ended episode."""
    from nclone_amd.engine import NppBatch

    r = golden.z("routes")
    name = golden.names("routes")[k]
    plan, marks = r["a%d" % k], r["t%d" % k]
    ck = {int(s): c for c, s in enumerate(r["cs%d" % k])}
    n = 64
    b = NppBatch(n, autoreset=True, fast_reset=False)
    b.load_levels([r["m%d" % k]])
    b.assign_levels(np.zeros(n, dtype=np.int32))
    b.set_routes(320)
    d_plan = torch.from_numpy(np.repeat(plan[:, None], n, axis=1)).cuda()
    start = seen = ended = 0
    for s in range(len(plan)):
        b.step(d_plan[s], 4)
        b.sync()
        flags = b.flags.cpu().numpy()
        term = (flags & 3) != 0
        assert term.all() == term.any() and bool(term[0]) == bool(marks[s]) and not (flags & 8).any(), (name, s, flags[0])
        if marks[s] or (s + 1) in ck:
            h, a = _routes(b)
            assert (h == h[0]).all(), (name, s)
        if marks[s]:
            for e in (0, n - 1):
                assert np.array_equal(_fin(h, a, e), plan[start:s + 1]), (name, s, e)
                assert h[e, 6:12].tolist()[:3] == [s + 1 - start, 0, 4] and h[e, 10] == flags[e] and h[e, 11] == 0, (name, s, h[e])
                assert h[e, :6].tolist() == ref.EMPTY, (name, s, h[e])
            start = s + 1
            ended += 1
        elif (s + 1) in ck:
            c = ck[s + 1]
            cl = int(r["cl%d" % k][c])
            assert cl == s + 1 - start
            f, di = b.dump_state()
            for e in (0, n - 1):
                assert np.array_equal(_cur(h, a, e), plan[s + 1 - cl:s + 1]), (name, s, e)
                assert h[e, :6].tolist() == [cl, 0, 4, int(r["cf%d" % k][c]), int(flags[e]), 0], (name, s, h[e])
                assert di[e, 22] == h[e, 3], (name, s)
                got = f[e, :2].astype(np.float32).astype(np.float64)
                want = r["cp%d" % k][c].astype(np.float32).astype(np.float64)
                assert np.abs(got - want).max() <= POS_TOL, (name, s, f[e, :2], r["cp%d" % k][c])
                if not name.startswith("zoo:"):   # (the step-boundary rows of test_rollouts_step_api_matches_reference: bit for bit)
                    assert np.array_equal(f[e, :2], r["cp%d" % k][c]) and np.array_equal(f[e, 2:4], r["cv%d" % k][c]), (name, s)
                assert (di[e, 13] != 1) == bool(r["cw%d" % k][c]), (name, s)
            seen += 1
    assert seen == len(ck) and ended == int(marks.sum()) >= 2
    b.close()


@pytest.mark.parametrize("which", ["mine", "door", "zoo"])
def test_a_route_reproduces_its_state(which):
    levels = _levels(which)
    b = _batch(levels)
    b.reset()
    acts = _acts(11, 40)
    for t in range(40):
        b.step(acts[t])
    assert b.archive_store(SRC_ENVS, SRC_SLOTS, status=True).cpu().numpy().tolist() == [0, 0, 0]
    at_store = _full(b, SRC_ENVS)
    ract, rhdr = b.archive_route_views()
    b.sync()
    rhdr, ract = rhdr.cpu().numpy(), ract.cpu().numpy()
    h, a = _routes(b)
    b.close()
    b2 = _batch(levels, slots=0)
    replayed = 0
    for env, slot in zip(SRC_ENVS, SRC_SLOTS):
        hd = rhdr[slot]
        route = ract[slot, :hd[0]]
        assert hd[6:].tolist() == [0, 0] and np.array_equal(hd[:6], h[env, :6]) and np.array_equal(route, _cur(h, a, env)), (env, hd)
        if hd[0] == 0:   # (the env's episode ended at the very step of the store: nothing to replay)
            continue
        replayed += 1
        assert hd[0] <= 40 and hd[1] == 0 and hd[2] == 4 and hd[5] == LEVEL_IDS[env] and hd[3] == at_store["i"][env, 22], (env, hd)
        assert np.array_equal(route, acts[40 - hd[0]:, env].cpu().numpy()), env
        b2.reset()
        b2.step_many(torch.from_numpy(np.repeat(route[:, None], N, axis=1)).cuda(), 4)
        got = _full(b2, [env])
        assert _rows_equal(got, env, at_store, env), (which, env, got["f"][env], at_store["f"][env])
        h2, a2 = _routes(b2)
        assert np.array_equal(h2[env, :6], hd[:6]) and np.array_equal(_cur(h2, a2, env), route), (env, h2[env])
    assert replayed >= 2
    b2.close()


def test_restore_carries_the_route():
    b = _batch(_levels("mine"))
    m = Model(b, CAP)
    b.reset()
    acts = _acts(5, 40)
    for t in range(20):
        b.step(acts[t])
        m.step(acts[t], 4)
    assert b.archive_store(SRC_ENVS, SRC_SLOTS, status=True).cpu().numpy().tolist() == [0, 0, 0]
    for t in range(20, 25):
        b.step(acts[t])
        m.step(acts[t], 4)
    before_h, before_a = m.check("before the restore")
    ract, rhdr = b.archive_route_views()
    b.sync()
    rhdr, ract = rhdr.cpu().numpy(), ract.cpu().numpy()
    # three good entries (same block, another block of the level, level 1) and one of every failure: another level, an empty
    # slot, a slot out of range
    envs, slots = [10, 150, 100, 71, 20, 21], [5, 5, 0, 5, 7, 99]
    assert b.archive_restore(envs, slots, status=True).cpu().numpy().tolist() == [0, 0, 0, 2, 3, 4]
    h, a = _routes(b)
    for env, slot in zip(envs[:3], slots[:3]):
        assert np.array_equal(h[env, :6], rhdr[slot, :6]) and np.array_equal(_cur(h, a, env), ract[slot, :rhdr[slot, 0]]), env
        assert np.array_equal(h[env, 6:], before_h[env, 6:]) and np.array_equal(_fin(h, a, env), _fin(before_h, before_a, env)), env
        m.r[env].restore(rhdr[slot, :6], ract[slot])
    touched = np.zeros(N, dtype=bool)
    touched[envs[:3]] = True
    assert np.array_equal(h[~touched], before_h[~touched]) and np.array_equal(a[~touched], before_a[~touched])
    m.check("after the restore")
    ends = np.zeros(N, dtype=bool)
    for t in range(25, 40):
        b.step(acts[t])
        flags, _ = m.step(acts[t], 4)
        ends |= (flags & 11) != 0
    h, a = m.check("15 steps later")
    for env, slot in zip(envs[:3], slots[:3]):
        if not ends[env]:
            want = np.concatenate([ract[slot, :rhdr[slot, 0]], acts[25:40, env].cpu().numpy()])
            assert np.array_equal(_cur(h, a, env), want), env
    b.close()


def test_a_won_episode_is_kept(golden):
    from nclone_amd.replay import decode_input_to_controls, route_to_replay, validate_replays
    from nclone_amd.vec_env import ACTION_TABLE

    c = golden.z("corpus")
    final = c["final"]
    won = [i for i in range(len(final)) if int(final[i, 1]) == 8]
    i = min(won, key=lambda j: int(final[j, 0]))
    T = int(final[i, 0])
    controls = [decode_input_to_controls(x) for x in c["in%d" % i][:T]]
    actions = np.array([ACTION_TABLE.index((hz, jp)) for hz, jp in controls], dtype=np.uint8)
    n = 64
    b = _batch([c["m%d" % i]], cap=(T + 15) // 16 * 16, n=n, level_ids=np.zeros(n, dtype=np.int32), slots=0)
    b.set_truncation_limit(10000)
    d = torch.from_numpy(np.repeat(actions[:, None], n, axis=1)).cuda()
    for t in range(T):
        b.step(d[t], 1)
    b.sync()
    assert (b.flags.cpu().numpy() & 1).all()   # won at the replay's last tick; the kernel has auto-reset every env
    h, a = _routes(b)
    for e in (0, n - 1):
        assert h[e, :6].tolist() == ref.EMPTY and h[e, 6:12].tolist()[:4] == [T, 0, 1, T] and h[e, 10] & 1, h[e]
        got = _fin(h, a, e)
        assert [ACTION_TABLE[x] for x in got] == controls
    rep = route_to_replay(c["m%d" % i], _fin(h, a, 0), h[0, 8], bool(h[0, 10] & 1))
    b.close()
    res = validate_replays([rep])[0]
    assert res["won"] and res["ticks"] == T and rep.success, res


def test_bits():
    levels = _levels("door")
    acts = _acts(9, 21)
    runs = {}
    for cap in (16, 64):
        b = _batch(levels, cap=cap, slots=0)
        m = Model(b, cap)
        b.reset()
        ends = np.zeros(N, dtype=bool)
        total = np.zeros(N, dtype=np.int64)
        for t in range(20):
            b.step(acts[t])
            flags, frames = m.step(acts[t], 4)
            ends |= (flags & 11) != 0
            total += frames
        h, a = m.check("cap %d" % cap)
        runs[cap] = (h, a, ends, total, b, m)
    h16, a16, ends, total, b, m = runs[16]
    h64, a64 = runs[64][:2]
    alive = np.flatnonzero(~ends)
    assert len(alive) > 0
    assert (h16[alive, 0] == 16).all() and (h16[alive, 1] == 1).all() and (h16[alive, 3] == total[alive]).all() and (total[alive] == 80).all()
    assert (h64[alive, 0] == 20).all() and (h64[alive, 1] == 0).all()
    assert np.array_equal(a16, a64[:, :, :16])   # nothing was written past a full buffer: other buffer and neighbours as in the wide run
    runs[64][4].close()
    # a step with another frame_skip: bit 2 on every route that was not empty
    nonempty = (h16[:, 0] > 0) | (h16[:, 1] != 0)
    b.step(acts[20], 2)
    flags, frames = m.step(acts[20], 2)
    h, a = m.check("frame_skip 2")
    hit = nonempty & (frames > 0) & ((flags & 11) == 0)
    assert hit.any() and (h[hit, 1] & 2).all() and (h[hit, 2] == 4).all()
    # raw ticks: bit 2 everywhere
    b.tick(torch.zeros((1, N), dtype=torch.uint8, device="cuda"))
    for r in m.r:
        r.tick()
    h, a = m.check("tick")
    assert (h[:, 1] & 2).all()
    # a flip clears the bits of the new current route and keeps them on the finished one
    b.reset()
    for r in m.r:
        r.reset()
    h2, a2 = m.check("reset")
    assert (h2[:, :6] == np.array(ref.EMPTY)).all() and np.array_equal(h2[:, 6:12], h[:, :6]) and np.array_equal(h2[:, 12], 1 - h[:, 12])
    b.close()


def test_one_rule_on_every_path(golden):
    from nclone_amd import _native as nat

    r = golden.z("routes")
    k = golden.names("routes").index("mines:hcorr:mines:100001")
    plan = r["a%d" % k]
    acts = np.stack([np.roll(plan, -e)[:30] for e in range(N)], axis=1).astype(np.uint8)   # env e starts the plan at action e
    d = torch.from_numpy(acts).cuda()
    got = {}
    for way in ("single", "many", "overlap", "no_rows"):
        b = _batch([r["m%d" % k]], level_ids=np.zeros(N, dtype=np.int32), slots=0)
        b.set_step_variant(0)   # (a pinned build: a split step needs no autotuner decision first; same bits)
        b.reset()
        if way == "overlap":
            b.set_obs_overlap(50)
        if way == "many":
            flags, _rew, _frames = b.step_many(d, 4)
            assert ((flags & 11) != 0).any()   # the 30 actions contain episode ends
        elif way == "no_rows":
            out = nat.StepOut()
            C.memmove(C.byref(out), C.byref(b._out), C.sizeof(nat.StepOut))
            out.d_flags, out.d_frames = None, None
            for t in range(30):
                nat.check(b.h, b.lib.npp_step(b.h, C.c_void_p(d[t].data_ptr()), 4, C.byref(out)))
        else:
            m = Model(b, CAP) if way == "single" else None
            for t in range(30):
                b.step(d[t])
                if m:
                    m.step(d[t], 4, np.zeros(N, dtype=np.int32))
            if m:
                m.check("single")
        got[way] = _routes(b)
        b.close()
    h, a = got["single"]
    assert (h[:, 6] > 0).any()
    for way in ("many", "overlap", "no_rows"):
        assert np.array_equal(got[way][0], h) and np.array_equal(got[way][1], a), way


def test_resets_flip(golden):
    levels = _levels("mine")
    b = _batch(levels, slots=0)
    m = Model(b, CAP)
    b.reset()
    acts = _acts(13, 30)
    for t in range(10):
        b.step(acts[t])
        m.step(acts[t], 4)
    rng = np.random.default_rng(2)
    mask_a, mask_b = (rng.random(N) < 0.4).astype(np.uint8), (rng.random(N) < 0.5).astype(np.uint8)
    b.reset(mask_a)   # (these envs then have an empty route: the second reset must leave them alone)
    for e in np.flatnonzero(mask_a):
        m.r[e].reset()
    h0, a0 = m.check("first masked reset")
    b.reset(mask_b)
    for e in np.flatnonzero(mask_b):
        m.r[e].reset()
    h1, a1 = m.check("second masked reset")
    flipped = (mask_b != 0) & ((h0[:, 0] > 0) | (h0[:, 1] != 0))
    assert flipped.any() and (~flipped & (mask_b != 0)).any()
    assert np.array_equal(h1[~flipped], h0[~flipped]) and np.array_equal(h1[flipped, 6:12], h0[flipped, :6])
    assert np.array_equal(h1[flipped, 12], 1 - h0[flipped, 12]) and np.array_equal(a1, a0)
    for t in range(10, 15):
        b.step(acts[t])
        m.step(acts[t], 4)
    # npp_assign_levels: the listed envs (here: to the level they play, so the model's levels stay)
    listed = np.flatnonzero(rng.random(N) < 0.3).astype(np.int32)
    b.assign_levels(LEVEL_IDS[listed], env_ids=listed)
    for e in listed:
        m.r[e].reset()
    h2, _ = m.check("assign_levels")
    assert (h2[listed, 0] == 0).all() and (h2[listed, 6] > 0).any()
    b.load_levels(levels)
    h3, _ = _routes(b)
    assert (h3 == np.array(EMPTY_HDR)).all()
    b.close()
    # level pool: a finished route keeps the level it was played on while the env moves to another
    b = _batch(levels, slots=0)
    b.set_level_pool([1.0, 1.0], seed=3)
    m = Model(b, CAP)
    b.reset()
    moved = 0
    for t in range(30):
        before = b.env_levels()
        b.step(acts[t])
        flags, _ = m.step(acts[t], 4, before)
        after = b.env_levels()
        h, a = _routes(b)
        for e in np.flatnonzero((flags & 11) != 0):
            assert h[e, 11] == before[e], (t, e)
            moved += int(after[e] != before[e])
    m.check("pool")
    assert moved > 0
    before = b.env_levels()
    b.draw_levels()
    for e in np.flatnonzero(b.env_levels() != before):
        m.r[e].reset()
    m.check("draw_levels")
    b.close()


def test_cell_index_slots_replay():
    levels = _levels("mine")
    b = _batch(levels, slots=256)
    b.archive_cells_create(seed=1)
    b.reset()
    acts = _acts(17, 60)
    for t in range(60):
        b.step(acts[t])
        if (t + 1) % 10 == 0:
            b.archive_explore()
    ract, rhdr = b.archive_route_views()
    meta = {k: v.cpu().numpy() for k, v in b.archive_meta().items()}
    b.sync()
    rhdr, ract = rhdr.cpu().numpy(), ract.cpu().numpy()
    b.close()
    ok = (meta["stored"] != 0) & (rhdr[:, 0] > 0) & (rhdr[:, 1] == 0)
    picks = [int(np.flatnonzero(ok & (meta["level"] == lvl))[-1]) for lvl in (0, 1)]
    b2 = _batch(levels, slots=0)
    for s in picks:
        route = ract[s, :rhdr[s, 0]]
        assert rhdr[s, 5] == meta["level"][s] and rhdr[s, 3] == meta["frame"][s] and rhdr[s, 2] == 4, (s, rhdr[s])
        b2.reset()
        b2.step_many(torch.from_numpy(np.repeat(route[:, None], N, axis=1)).cuda(), 4)
        f, di = b2.dump_state()
        e = 3 if meta["level"][s] == 0 else 70
        assert np.array_equal(f[e, :4], [meta[c][s] for c in ("x", "y", "vx", "vy")]), (s, f[e, :4])
        assert di[e, 22] == meta["frame"][s] and int(di[e, 13] != 1) == meta["switch_activated"][s], s
    b2.close()


def test_layout_and_refusals():
    from nclone_amd import _native as nat

    b = _batch(_levels("mine"), cap=0)
    plain = b.archive_record_bytes()
    for call in (b.route_views, b.archive_route_views):   # the feature is off
        with pytest.raises(nat.NppError) as ei:
            call()
        assert ei.value.code == nat.NPP_ERR_STATE
    with pytest.raises(nat.NppError) as ei:
        b.set_routes(CAP)   # while an archive exists
    assert ei.value.code == nat.NPP_ERR_STATE
    b.archive_create(0)
    with pytest.raises(ValueError):
        b.set_routes(-1)
    assert b.lib.npp_set_routes(b.h, -1) == nat.NPP_ERR_INVALID
    b.set_routes(CAP - 3)   # rounded up to a multiple of 16
    assert b.route_views()[0].shape == (N, 2, CAP)
    b.archive_create(SLOTS)
    assert b.archive_record_bytes() - plain == 32 + CAP
    act, hdr = b.archive_route_views()
    assert act.shape == (SLOTS, CAP) and hdr.shape == (SLOTS, 8) and act.data_ptr() - hdr.data_ptr() == 32
    b.archive_create(0)
    b.snapshot()
    b.restore()
    b.set_routes(32)
    with pytest.raises(nat.NppError) as ei:
        b.restore()   # the snapshot's records were laid out for the old capacity
    assert ei.value.code == nat.NPP_ERR_STATE
    # the snapshot slot carries the route like any record
    acts = _acts(1, 12)
    b.reset()
    for t in range(6):
        b.step(acts[t])
    b.snapshot()
    h0, a0 = _routes(b)
    for t in range(6, 12):
        b.step(acts[t])
    b.restore()
    h1, a1 = _routes(b)
    assert np.array_equal(h1[:, :6], h0[:, :6])
    for e in range(N):
        assert np.array_equal(_cur(h1, a1, e), _cur(h0, a0, e)), e
    b.set_routes(0)
    with pytest.raises(nat.NppError):
        b.route_views()
    b.close()


@pytest.mark.parametrize("output", ["torch", "numpy"])
def test_host_classes(golden, output):
    from nclone_amd.vec_env import NppEnvironment, NppVecEnvironment

    r = golden.z("routes")
    k = golden.names("routes").index("mines:hcorr:mines:100001")
    plan = r["a%d" % k]
    levels = [r["m%d" % k], _levels("mine")[0]]
    v = NppVecEnvironment(levels, N, record_routes=True, route_capacity=CAP, checkpoint_slots=SLOTS, output=output, fast_reset=False,
                          truncation_limit=10000)
    v.reset()
    acts = np.stack([np.roll(plan, -e)[:40] for e in range(N)], axis=1).astype(np.uint8)
    cur = [[] for _ in range(N)]
    fin = [None] * N
    for t in range(40):
        _obs, _rew, term, trunc, info = v.step(acts[t])
        done = np.asarray((term | trunc).cpu() if output == "torch" else (term | trunc))
        frames = np.asarray(info["frames_executed"].cpu() if output == "torch" else info["frames_executed"])
        for e in range(N):
            if frames[e] > 0:
                cur[e].append(int(acts[t, e]))
            if done[e]:
                fin[e], cur[e] = cur[e], []
    lens = v.get_action_sequence_length()
    assert isinstance(lens, torch.Tensor if output == "torch" else np.ndarray)
    assert np.asarray(lens.cpu() if output == "torch" else lens).tolist() == [len(c) for c in cur]
    for e in (0, 3, 70, 130, N - 1):
        seq = v.get_current_action_sequence(e)
        assert seq.dtype == np.uint8 and seq.tolist() == cur[e], e
    routes = {d["env"]: d for d in v.finished_routes()}
    assert sorted(routes) == [e for e in range(N) if fin[e] is not None] and len(routes) > 0
    for e, d in routes.items():
        assert d["actions"].tolist() == fin[e] and d["frame_skip"] == 4 and d["bits"] == 0 and d["flags"] & 11 and d["level"] == (e // 64) % 2, e
        assert 4 * (len(fin[e]) - 1) < d["frame_count"] <= 4 * len(fin[e]), e
    some = np.zeros(N, dtype=np.uint8)
    some[:64] = 1
    assert [d["env"] for d in v.finished_routes(some)] == [e for e in sorted(routes) if e < 64]
    # the archive: routes of slots, and a restart leaves the slot's route
    slot_ids = np.full(N, -1, dtype=np.int32)
    slot_ids[3], slot_ids[70] = 5, 0
    st = v.archive_store(slot_ids)
    assert int(st[3]) == 0 and int(st[70]) == 0
    got = v.archive_routes([5, 0, 7])
    meta = {key: val.cpu().numpy() for key, val in v.archive_meta().items()}
    assert got[2] is None
    for d, env, slot in ((got[0], 3, 5), (got[1], 70, 0)):
        assert d["actions"].tolist() == cur[env] and d["slot"] == slot and d["level"] == (env // 64) % 2 and d["frame_skip"] == 4 and d["bits"] == 0
        assert d["position"] == (meta["x"][slot], meta["y"][slot]) and d["velocity"] == (meta["vx"][slot], meta["vy"][slot])
        assert d["cell"] == (meta["cell_x"][slot], meta["cell_y"][slot]) and d["switch"] == bool(meta["switch_activated"][slot])
        assert d["frame_count"] == meta["frame"][slot]
    ract, rhdr = v.batch.archive_route_views()
    assert rhdr[5, 0].item() == len(cur[3]) and ract[5, :len(cur[3])].cpu().numpy().tolist() == cur[3]
    back = np.full(N, -1, dtype=np.int32)
    back[10], back[100] = 5, 0
    v.restart(back)
    assert v.get_current_action_sequence(10).tolist() == cur[3] and v.get_current_action_sequence(100).tolist() == cur[70]
    assert v.get_current_action_sequence(11).tolist() == cur[11]
    # a checkpoint replay leaves the replayed sequence as the route (base_environment.py:2114)
    s = [2, 2, 5, 0, 1, 3, 2]
    _obs, info = v.reset(options={"checkpoint": {"action_sequence": s}})
    dead = np.asarray(info["replay_terminated"].cpu())
    assert not dead.all()
    for e in np.flatnonzero(~dead)[:4]:
        assert v.get_current_action_sequence(int(e)).tolist() == s, e
    v.close()
    if output == "numpy":
        env = NppEnvironment(map_data=levels[0], record_routes=True, route_capacity=CAP, truncation_limit=10000)
        env.reset()
        want = []
        for a in plan[:12]:
            _o, _r, term, trunc, _i = env.step(int(a))
            want.append(int(a))
            assert env.get_current_action_sequence() == want and env.get_action_sequence_length() == len(want)
            if term or trunc:
                env.reset()
                want = []
                assert env.get_current_action_sequence() == [] and env.get_action_sequence_length() == 0
        env.close()
