"""GPU tests of seeding the cell index from replays (include/npp_amd.h npp_archive_seed, nclone_amd/csrc/npp_seed.hip)
against the restatement (tests/seed_ref.py), which builds the expected tables from the checkpoints the REFERENCE's seeder returned
(tests/golden/seed.npz).  Base shape: N = 3 envs on the three levels of the fixture's first three replays, 64 slots, routes on with
capacity 128, frame skip 1.  The restatements are computed once per shape and shared."""
import ctypes as C

import numpy as np
import pytest

from tests import cell_archive_ref as cref
from tests import seed_ref as sref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

POS_TOL = 1e-5   # tests/test_gpu_demo.py: the bar on float32 positions
_cache = {}


def _reps():
    if "reps" not in _cache:
        _cache["z"] = sref.fixture()
        _cache["reps"] = sref.Replays(_cache["z"])
    return _cache["z"], _cache["reps"]


def _expected(n, slots=64, mode="progress", table=None, tag=None):
    key = (n, slots, mode, tag)
    if key not in _cache:
        _cache[key] = sref.Expected(_reps()[1], n, slots, mode, table)
    return _cache[key]


def _env(n=3, slots=64, cap=128, levels=None, cells=True, **kw):
    from nclone_amd.vec_env import NppVecEnvironment

    levels = _reps()[1].levels if levels is None else levels
    return NppVecEnvironment(levels, n, level_ids=np.arange(n) % len(levels), frame_skip=1, truncation_limit=10000, checkpoint_slots=slots,
                             checkpoint_cells=cells, record_routes=cap > 0, route_capacity=cap if cap > 0 else None, **kw)


def _tables(env):
    t = {k: v.cpu().numpy().reshape(-1).copy() for k, v in env.batch.archive_cells().items()}
    t["cell_score"] = t["cell_score"].view(np.uint32)
    return t


def _meta(env):
    return {k: v.cpu().numpy().copy() for k, v in env.archive_meta().items()}


def _assert_tables(env, X, what):
    t = _tables(env)
    want = {"cell_slot": X.cell_slot, "cell_score": X.cell_score.view(np.uint32), "slot_key": X.slot_key,
            "n_used": np.array([X.n_used], dtype=np.int32)}
    for k, w in want.items():
        assert np.array_equal(t[k], w), (what, k, np.nonzero(t[k] != w)[0][:8])
    assert not t["visits"].any() and not t["chosen"].any(), what   # the seeder adds cells, not visits
    return t


def _assert_meta(env, X, what):
    """The occupied slots hold the reference's positions (inside the position bar), with frame, level, cell and switch exact."""
    z, reps = _reps()
    m = _meta(env)
    worst = 0.0
    for s in range(X.n_used):
        r, f = X.slot_src[s]
        _, pos, sw = reps.ticks[r][f]
        got = np.array([m["x"][s], m["y"][s]])
        worst = max(worst, float(np.abs(got.astype(np.float32).astype(np.float64) - pos.astype(np.float32).astype(np.float64)).max()))
        assert m["stored"][s] == 1 and m["frame"][s] == f + 1 and m["switch_activated"][s] == sw and m["level"][s] == reps.level[r], (what, s)
        assert m["cell_x"][s] == np.floor(pos[0] / 24.0) and m["cell_y"][s] == np.floor(pos[1] / 24.0), (what, s)
    print("%s: %d slots, worst f32 position difference to the reference %.3g" % (what, X.n_used, worst))
    assert worst <= POS_TOL, what
    assert not m["stored"][X.n_used:].any(), what


@pytest.mark.parametrize("n", [3, 1, 8])
def test_tables_equal_the_restatement(n):
    """N = 3 (two rounds), 1 (six rounds) and 8 (one round, two idle envs): each against the restatement for ITS n, so the results
    differ between them only where the restatement says so (ties)."""
    z, reps = _reps()
    env = _env(n)
    out = env.seed_archive_from_replays(reps.compact())
    X = _expected(n)
    _assert_tables(env, X, "n=%d" % n)
    _assert_meta(env, X, "n=%d" % n)
    assert out["status"].cpu().tolist() == [0, 0, 0, 0, 0, 0, 1, 2] and out["cells"] == X.n_used
    assert np.array_equal(out["counts"].cpu().numpy(), X.counts), (out["counts"].cpu().numpy(), X.counts)
    # the handle is back on its levels with empty routes, and a reset serves observations
    assert env.batch.env_levels().tolist() == (np.arange(n) % 3).tolist()
    obs, _ = env.reset()
    assert env.get_action_sequence_length().cpu().tolist() == [0] * n and not env.finished_routes()
    assert torch.isfinite(obs["game_state"]).all()
    env.close()


def test_max_demos_per_level_and_paths(tmp_path):
    """max_demos_per_level = 1 keeps the first replay of every level in the caller's order (status 3 for the rest); paths work."""
    z, reps = _reps()
    paths = []
    for k, r in enumerate(reps.compact()):
        p = tmp_path / ("r%d.replay" % k)
        p.write_bytes(r.to_binary())
        paths.append(str(p))
    env = _env(3)
    out = env.seed_archive_from_replays(paths, max_demos_per_level=1)
    assert out["status"].cpu().tolist() == [0, 0, 0, 3, 3, 3, 1, 2]
    capped = sref.Replays(z, max_per_level=1)
    X = sref.Expected(capped, 3, 64)
    _assert_tables(env, X, "capped")
    assert np.array_equal(out["counts"].cpu().numpy(), X.counts)
    env.close()


def _routes_by_slot(env, X):
    return env.archive_routes(np.arange(X.n_used))


def test_routes_of_seeded_slots():
    z, reps = _reps()
    env = _env(3)
    env.seed_archive_from_replays(reps.compact())
    X = _expected(3)
    t7 = int(z["byte7_tick"][0])
    routes = _routes_by_slot(env, X)
    behind7 = 0
    for s, d in enumerate(routes):
        r, f = X.slot_src[s]
        want = sref.route_of(reps.inputs[r], f)
        assert np.array_equal(d["actions"], want) and len(d["actions"]) == f + 1, s
        assert d["frame_skip"] == 1 and d["frame_count"] == f + 1 and d["level"] == reps.level[r], s
        broken = r == 5 and f >= t7
        behind7 += int(broken)
        assert d["bits"] == (2 if broken else 0), (s, r, f, d["bits"])
    assert behind7 >= 1   # a slot reached after the byte-7 tick, and only such slots carry bit 2
    # an env restarted from a seeded slot has the slot's position and the slot's route as its own
    env.reset()
    meta = _meta(env)
    pick = []
    for e in range(3):   # the slot of level e with the longest route (level 1's only cell belongs to the byte-7 replay)
        mine = [s for s in range(X.n_used) if reps.level[X.slot_src[s][0]] == e]
        pick.append(max(mine, key=lambda s: X.slot_src[s][1]))
    replayable = [e for e, s in enumerate(pick) if routes[s]["bits"] == 0]
    assert replayable == [0, 2]
    obs = env.restart(np.array(pick, dtype=np.int32))
    px, py = obs["player_x"].cpu().numpy().copy(), obs["player_y"].cpu().numpy().copy()
    for e, s in enumerate(pick):
        assert px[e] == meta["x"][s] and py[e] == meta["y"][s], e
        assert np.array_equal(env.get_current_action_sequence(e), routes[s]["actions"]), e
    # replaying a route without bit 2 with step() at frame skip 1 from a reset reaches the same position
    env.reset()
    lens = [len(routes[s]["actions"]) for s in pick]
    for t in range(max(lens)):
        acts = np.array([routes[s]["actions"][t] if t < len(routes[s]["actions"]) else 0 for s in pick], dtype=np.uint8)
        obs, _, _, _, _ = env.step(acts)
        x, y = obs["player_x"].cpu().numpy(), obs["player_y"].cpu().numpy()
        for e, s in enumerate(pick):
            if t == lens[e] - 1 and e in replayable:
                assert x[e] == meta["x"][s] and y[e] == meta["y"][s], (e, t, x[e], meta["x"][s])
    env.close()


def test_route_capacity_16():
    z, reps = _reps()
    env = _env(3, cap=16)
    env.seed_archive_from_replays(reps.compact())
    X = _expected(3)
    _assert_tables(env, X, "cap 16")
    over = 0
    for s, d in enumerate(_routes_by_slot(env, X)):
        r, f = X.slot_src[s]
        assert bool(d["bits"] & 1) == (f + 1 > 16), (s, f)
        assert np.array_equal(d["actions"], sref.route_of(reps.inputs[r], f)[:16]) and d["frame_count"] == f + 1, s
        over += int(f + 1 > 16)
    assert 0 < over
    env.close()


def test_archive_full():
    z, reps = _reps()
    env = _env(3, slots=8)
    out = env.seed_archive_from_replays(reps.compact())
    F = _expected(3, slots=8)
    _assert_tables(env, F, "8 slots")
    _assert_meta(env, F, "8 slots")
    counts = out["counts"].cpu().numpy()
    assert np.array_equal(counts, F.counts) and int(counts[:, 3].sum()) == F.overflow > 0 and out["cells"] == 8
    # the first 8 new cells in call order hold the slots
    X = _expected(3)
    firsts = [int(X.slot_key[slot]) for _, _, slot, old in X.events if old < 0][:8]
    assert _tables(env)["slot_key"].tolist() == firsts
    env.close()


def test_score_frames_equals_an_explore_loop():
    """score="frames" against the same ticks played by hand through tick() + archive_explore(score=None, mask=candidates): the same
    tables and meta rows, except that the loop's visits count and the seeding's stay zero.  Routes off: nothing route-related runs."""
    from nclone_amd import demos

    z, reps = _reps()
    env = _env(3, cap=0)
    env.seed_archive_from_replays(reps.compact(), score="frames")
    X = _expected(3, mode="frames")
    seeded = _assert_tables(env, X, "frames")
    seeded_meta = _meta(env)
    env.close()
    hand = _env(3, cap=0)
    b = hand.batch
    lengths = np.array([len(reps.inputs[r]) for r in reps.played], dtype=np.int64)
    plan = demos.plan(lengths, 1, int(lengths.max()), 3)
    order = [reps.played[k] for k in plan["order"]]
    for q, ticks in enumerate(plan["round_ticks"]):
        envs = order[q * 3:(q + 1) * 3]
        b.assign_levels([reps.level[envs[e] if e < len(envs) else envs[0]] for e in range(3)])
        b.reset(mode="full")
        rows = np.zeros((int(ticks), 3), dtype=np.uint8)
        for e, r in enumerate(envs):
            rows[:len(reps.inputs[r]), e] = reps.inputs[r]
        d_rows = torch.from_numpy(rows).cuda()
        for f in range(int(ticks)):
            b.tick(d_rows[f:f + 1])
            b.archive_explore(score=None, mask=np.array([e < len(envs) and f < len(reps.inputs[envs[e]]) for e in range(3)], dtype=np.uint8))
    loop = _tables(hand)
    for k in ("cell_slot", "cell_score", "slot_key", "n_used"):
        assert np.array_equal(loop[k], seeded[k]), k
    assert loop["visits"].sum() == X.counts[:, 1].sum() > 0   # one visit per eligible tick there, none here
    loop_meta = _meta(hand)
    for k in seeded_meta:
        assert np.array_equal(loop_meta[k], seeded_meta[k]), k
    hand.close()


def test_score_table_and_nan():
    """A caller's table of -progress picks the EARLIEST frame per cell; a NaN entry is skipped."""
    z, reps = _reps()
    table = {r: (-(np.arange(len(reps.inputs[r]), dtype=np.float64) / len(reps.inputs[r]))).astype(np.float32) for r in range(len(reps.maps))}
    env = _env(3)
    scores = [torch.from_numpy(table[r]).cuda() if r % 2 else table[r] for r in range(len(reps.maps))]   # tensors and arrays
    scores[7] = None   # (not played)
    env.seed_archive_from_replays(reps.compact(), score=scores)
    X = _expected(3, mode="table", table=table, tag="neg")
    _assert_tables(env, X, "table")
    _assert_meta(env, X, "table")
    for s in range(X.n_used):
        r, f = X.slot_src[s]
        k = int(X.slot_key[s])
        assert f == min(g for g, (kk, _, _) in reps.ticks[r].items() if kk == k), s
    env.close()
    # NaN at a winning entry: the cell goes to the next best tick, and the tick is not eligible
    s0 = next(s for s in range(X.n_used) if X.slot_src[s][0] == 2)
    r, f = X.slot_src[s0]
    holed = {q: v.copy() for q, v in table.items()}
    holed[r][f] = np.nan
    env = _env(3)
    out = env.seed_archive_from_replays(reps.compact(), score=[holed[q] for q in range(len(reps.maps))])
    Y = _expected(3, mode="table", table=holed, tag="nan")
    _assert_tables(env, Y, "nan")
    counts = out["counts"].cpu().numpy()
    assert np.array_equal(counts, Y.counts) and counts[r, 1] == X.counts[r, 1] - 1 and counts[r, 0] == X.counts[r, 0]
    assert (r, f) not in Y.slot_src.values()
    env.close()


def test_seeding_is_invisible_to_the_episodes_that_follow():
    """Two envs with the same levels and actions under reward_mode="pbrs" (and hard action masking): one seeds before reset(), the
    other does not; twenty steps give bit-identical observations, rewards and flags."""
    z, reps = _reps()
    levels = reps.levels[:2]   # (exit switch + door only: levels the mode accepts)
    acts = np.random.default_rng(4).integers(0, 6, size=(20, 4)).astype(np.uint8)
    runs = []
    for seed_it in (True, False):
        env = _env(4, levels=levels, reward_mode="pbrs", action_masking_mode="hard")
        if seed_it:
            out = env.seed_archive_from_replays(reps.compact())
            assert out["cells"] > 0 and out["status"].cpu().tolist() == [0, 0, 1, 0, 0, 0, 1, 2]
        obs, info = env.reset(seed=9)
        rows = [{k: v.clone() for k, v in obs.items()}]
        for t in range(20):
            obs, rew, term, trunc, info = env.step(acts[t])
            rows.append(dict({k: v.clone() for k, v in obs.items()}, reward=rew.clone(), terminated=term.clone(), truncated=trunc.clone(),
                             path_direction=info["path_direction"].clone(), pbrs=info["pbrs_components"].clone()))
        runs.append(rows)
        env.close()
    for t, (a, b) in enumerate(zip(*runs)):
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(_bits(a[k]), _bits(b[k])), (t, k)


def _bits(t):
    t = t.contiguous()
    return t if t.dtype == torch.bool else t.view(torch.uint8)


def _direct(env, inputs, offsets, levels, mode, scores=None):
    b = env.batch
    inp, off, lv = np.ascontiguousarray(inputs, dtype=np.uint8), np.ascontiguousarray(offsets, dtype=np.int64), np.ascontiguousarray(levels, dtype=np.int32)
    with b._ctx():
        return b.lib.npp_archive_seed(b.h, inp.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p), lv.ctypes.data_as(C.c_void_p), len(lv),
                                      mode, None if scores is None else C.c_void_p(scores.data_ptr()), None)


def test_refusals_leave_the_index_untouched():
    from nclone_amd import _native as nat
    from nclone_amd._native import NppError

    z, reps = _reps()
    small = sref.Replays(z, load=(0, 1))   # (exit switch + door only: levels reward mode "pbrs" accepts)
    env = _env(3, levels=small.levels)
    env.seed_archive_from_replays(reps.compact())
    X = sref.Expected(small, 3, 64)
    before, meta_before = _assert_tables(env, X, "before"), _meta(env)
    b = env.batch
    inp = reps.inputs[0]
    good = (inp, [0, len(inp)], [0])
    assert _direct(env, inp, [1, len(inp)], [0], 0) == nat.NPP_ERR_INVALID           # offsets[0] != 0
    assert _direct(env, inp, [0, len(inp)], [3], 0) == nat.NPP_ERR_INVALID           # level id out of range
    assert _direct(env, inp, [0, len(inp)], [-1], 0) == nat.NPP_ERR_INVALID
    assert _direct(env, inp, [0, 5, 2], [0, 0], 0) == nat.NPP_ERR_INVALID            # a negative length
    assert _direct(env, *good, 3) == nat.NPP_ERR_INVALID                              # an unknown mode
    assert _direct(env, *good, 2) == nat.NPP_ERR_INVALID                              # mode 2 without d_scores
    with pytest.raises(ValueError, match="score_mode"):
        b.archive_seed(*good, "returns")
    with pytest.raises(ValueError, match="one array per replay"):
        env.seed_archive_from_replays(reps.compact(), score="returns")
    b.set_action_masking("hard")
    assert _direct(env, *good, 0) == nat.NPP_ERR_STATE and b"action masking" in b.lib.npp_last_error(b.h)
    b.set_action_masking(None)
    b.set_reward_mode("pbrs")
    with pytest.raises(NppError, match="pbrs"):
        b.archive_seed(*good, "progress")
    b.set_reward_mode("sparse")
    after = _tables(env)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    meta_after = _meta(env)
    for k in meta_before:
        assert np.array_equal(meta_before[k], meta_after[k]), k
    assert env.batch.env_levels().tolist() == [0, 1, 0]
    env.close()
    # without a cell index
    plain = _env(3, cells=False)
    with pytest.raises(RuntimeError, match="checkpoint_cells"):
        plain.seed_archive_from_replays(reps.compact())
    assert _direct(plain, *good, 0) == nat.NPP_ERR_STATE and b"no cell index" in plain.batch.lib.npp_last_error(plain.batch.h)
    plain.close()
    # options the env method cannot lift are named
    stacked = _env(3, enable_state_stacking=True)
    with pytest.raises(NotImplementedError, match="enable_state_stacking"):
        stacked.seed_archive_from_replays(reps.compact())
    assert not _tables(stacked)["n_used"][0]
    stacked.close()


def test_explore_on_a_seeded_index():
    """npp_archive_explore behaves as before on a seeded index: an env with a higher score takes a seeded cell, and visits count
    from zero."""
    z, reps = _reps()
    env = _env(3)
    env.seed_archive_from_replays(reps.compact())
    X = _expected(3)
    env.reset()
    env.step(np.zeros(3, dtype=np.uint8))
    f, i = env.batch.dump_state()
    R = cref.CellArchiveRef([cref.door_of(m) for m in reps.levels], 64)
    keys = R.keys(f, i)
    assert (keys >= 0).all() and all(X.cell_slot[k] >= 0 for k in keys[:2])   # the spawn cells of the two small levels are seeded
    low = env.archive_explore(score=np.full(3, -5.0, dtype=np.float32)).cpu().numpy()
    t = _tables(env)
    for e in range(2):
        assert low[e] == cref.LOST and t["cell_score"][keys[e]] == X.cell_score.view(np.uint32)[keys[e]] and t["visits"][keys[e]] == 1
    high = env.archive_explore(score=np.full(3, 5.0, dtype=np.float32)).cpu().numpy()
    t = _tables(env)
    meta = _meta(env)
    for e in range(2):
        k = int(keys[e])
        assert high[e] == cref.STORED and t["cell_slot"][k] == X.cell_slot[k] and t["visits"][k] == 2
        assert t["cell_score"][k] == np.array([5.0], dtype=np.float32).view(np.uint32)[0]
        s = int(X.cell_slot[k])
        assert meta["x"][s] == f[e, 0] and meta["y"][s] == f[e, 1] and meta["frame"][s] == i[e, 22]
    assert t["visits"].sum() == 6 and not t["chosen"].any()
    env.close()
