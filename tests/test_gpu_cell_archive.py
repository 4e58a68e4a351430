"""GPU tests of the cell index over the checkpoint archive (include/npp_amd.h npp_archive_cells_create, nclone_amd/csrc/npp_cells.hip;
DESIGN.md 17) against the Python restatement of its rule (tests/cell_archive_ref.py): statuses, tables, meta rows and drawn slots are
compared exactly after every call.  The base shape is that of tests/test_gpu_archive.py: 192 envs, blocks 0 and 2 on level 0 and
block 1 on level 1, 64 slots.  Level 0 is a mine level whose exit switch lies close to the spawn and 84 px from its door -- a
random walk of 40 steps activates it in a good part of the envs, so switch_activated takes both values among the eligible states
without a fixture (asserted below) -- level 1 a door level whose switch lies 43 px from its door, so the states behind its switch
fall to the exit filter.  The 64 slots fill up during the 40-step walk when it visits more than 64 cells; the full path itself is pinned by the
1300-env test."""
import numpy as np
import pytest

from tests import cell_archive_ref as ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, SLOTS = 192, 64
LEVEL_IDS = (np.arange(N) // 64) % 2
TABLES = ("cell_slot", "cell_score", "visits", "chosen", "slot_key", "n_used")
_cache = {}


def _levels():
    if "levels" not in _cache:
        from nclone_amd import levels as lv

        _cache["levels"] = [lv.mine_levels()[0][45], lv.door_levels()[0][14]]
        _cache["doors"] = [ref.door_of(m) for m in _cache["levels"]]
    return _cache["levels"], _cache["doors"]


def _batch(levels=None, n=N, level_ids=LEVEL_IDS, slots=SLOTS, cells=True, seed=5):
    from nclone_amd.engine import NppBatch

    b = NppBatch(n, autoreset=True)
    b.load_levels(_levels()[0] if levels is None else levels)
    b.assign_levels(level_ids)
    if slots:
        b.archive_create(slots)
        if cells:
            b.archive_cells_create(seed=seed)
    b.reset()
    return b


def _acts(seed, steps, n=N):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 6, size=(steps, n)).astype(np.uint8)).cuda()


def _tables(b):
    """The index's tables as flat host arrays (scores as their bits, so that -0.0 is not +0.0)."""
    t = {k: v.cpu().numpy().reshape(-1).copy() for k, v in b.archive_cells().items()}
    t["cell_score"] = t["cell_score"].view(np.uint32)
    t["visits"], t["chosen"] = t["visits"].view(np.uint32), t["chosen"].view(np.uint32)
    return t


def _meta(b):
    m = {k: v.cpu().numpy() for k, v in b.archive_meta().items()}
    f = np.stack([m[k] for k in ("x", "y", "vx", "vy")], axis=1)
    i = np.stack([m[k] for k in ("stored", "level", "frame", "cell_x", "cell_y", "switch_activated")], axis=1)
    return f, i


def _assert_equals_ref(b, R, what):
    t = _tables(b)
    want = {"cell_slot": R.cell_slot, "cell_score": R.cell_score.view(np.uint32), "visits": R.visits, "chosen": R.chosen,
            "slot_key": R.slot_key, "n_used": np.array([R.n_used], dtype=np.int32)}
    for k in TABLES:
        assert np.array_equal(t[k], want[k]), (what, k, np.nonzero(t[k] != want[k])[0][:8])
    f, i = _meta(b)
    u = R.n_used
    assert np.array_equal(f[:u].view(np.uint64), R.slot_f[:u].view(np.uint64)) and np.array_equal(i[:u], R.slot_i[:u]), (what, "meta")
    assert not i[u:, 0].any(), (what, "stored beyond n_used")


def test_explore_right_after_reset():
    """All envs of a level share one cell and one score: the lowest env of each level wins it, everybody else loses the tie."""
    b = _batch()
    st = b.archive_explore(status=True).cpu().numpy()
    want = np.full(N, ref.LOST, dtype=np.int32)
    want[0] = want[64] = ref.STORED
    assert np.array_equal(st, want)
    t = _tables(b)
    f, i = b.dump_state()
    R = ref.CellArchiveRef(_levels()[1], SLOTS)
    k0, k1 = int(R.keys(f, i)[0]), int(R.keys(f, i)[64])
    assert 0 <= k0 < ref.CELLS_PER_LEVEL <= k1
    assert t["n_used"][0] == 2 and t["cell_slot"][k0] == 0 and t["cell_slot"][k1] == 1 and (t["cell_slot"] >= 0).sum() == 2
    assert t["visits"][k0] == 128 and t["visits"][k1] == 64 and t["visits"].sum() == N and not t["chosen"].any()
    assert t["slot_key"].tolist() == [k0, k1] + [-1] * (SLOTS - 2)
    mf, mi = _meta(b)
    for slot, e in ((0, 0), (1, 64)):
        assert np.array_equal(mf[slot], f[e, :4])
        assert mi[slot].tolist() == [1, i[e, 27], i[e, 22], int(np.floor(f[e, 0] / 24)), int(np.floor(f[e, 1] / 24)), int(i[e, 13] != 1)]
    assert np.array_equal(R.explore(f, i), st)
    _assert_equals_ref(b, R, "reset")
    b.close()


@pytest.mark.parametrize("mode,slots", [("frames", SLOTS), ("caller", 256)])
def test_random_walk_against_the_restatement(mode, slots):
    """Forty random steps with autoreset on, explore after every step.  "frames": score=None with the base shape's 64 slots, which
    fill up on the way (status 7 beside 0 and 6).  "caller": a caller's score with negative values, both zeros, repeated values,
    +inf and one NaN per call, and 256 slots so that cells behind an activated switch still find room (their meta rows are then
    compared too).  The switch is activated by the random walk itself, on level 0; no fixture state is restored."""
    b = _batch(slots=slots)
    R = ref.CellArchiveRef(_levels()[1], slots)
    acts = _acts(11, 40)
    rng = np.random.default_rng(12)
    values = np.array([-2.5, -1.0, -1.0, -0.0, 0.0, 0.5, 0.5, 3.0], dtype=np.float32)
    seen, sw_visited, visited, filtered = set(), set(), set(), 0
    for t in range(40):
        b.step(acts[t])
        f, i = b.dump_state()
        score = None
        if mode == "caller":
            score = values[rng.integers(0, len(values), N)]
            score[rng.integers(0, N)] = np.inf
            score[rng.integers(0, N)] = np.nan
        st = b.archive_explore(score=None if score is None else torch.from_numpy(score).cuda(), status=True).cpu().numpy()
        want = R.explore(f, i, score=score)
        assert np.array_equal(st, want), (t, np.nonzero(st != want)[0][:8])
        _assert_equals_ref(b, R, t)
        seen.update(st.tolist())
        keys = R.keys(f, i)
        visited.update(keys[keys >= 0].tolist())
        sw_visited.update(((keys[keys >= 0] % ref.CELLS_PER_LEVEL) // 1100).tolist())
        filtered += int(((keys < 0) & (i[:, 13] != 1) & (i[:, 0] <= 5)).sum())   # live, inside the grid, too near the door
    print("cells visited", len(visited), "switch planes", sw_visited, "states the exit filter dropped", filtered, "statuses", seen)
    assert sw_visited == {0, 1}, "the random walk no longer activates a switch: choose another level or seed"
    if mode == "frames":
        assert {ref.STORED, ref.LOST} <= seen and (ref.FULL in seen) == (len(visited) > slots) and R.n_used == min(len(visited), slots)
    else:
        assert {ref.STORED, ref.LOST, ref.NOT_ELIGIBLE} <= seen
        assert set(R.slot_i[:R.n_used, 5].tolist()) == {0, 1}   # stored cells on both sides of the switch
        assert set(R.slot_i[:R.n_used, 1].tolist()) == {0, 1}
    b.close()


def test_chunk_boundary_and_full_archive():
    """1300 envs on 1300 level entries (two maps alternating, one env per level) and 1200 slots: the smallest shape at which the
    assign kernel's chunk loop runs twice (the second chunk partial) and the archive fills inside a call."""
    n, slots = 1300, 1200
    maps, doors = _levels()
    b = _batch(levels=[maps[k % 2] for k in range(n)], n=n, level_ids=np.arange(n), slots=slots)
    R = ref.CellArchiveRef([doors[k % 2] for k in range(n)], slots)
    f, i = b.dump_state()
    st = b.archive_explore(status=True).cpu().numpy()
    assert np.array_equal(st[:slots], np.zeros(slots, dtype=np.int32)) and np.array_equal(st[slots:], np.full(n - slots, ref.FULL))
    keys = R.keys(f, i)
    assert np.array_equal(keys // ref.CELLS_PER_LEVEL, np.arange(n))
    t = _tables(b)
    assert np.array_equal(t["cell_slot"][keys[:slots]], np.arange(slots)) and np.array_equal(t["slot_key"], keys[:slots])
    assert (t["cell_slot"][keys[slots:]] == -1).all() and (t["visits"][keys] == 1).all() and t["n_used"][0] == slots
    assert np.array_equal(R.explore(f, i), st)
    _assert_equals_ref(b, R, "first")
    # a full key left no trace but its visit count: after one step the second call behaves as the restatement says
    b.step(_acts(13, 1, n)[0])
    f, i = b.dump_state()
    st = b.archive_explore(status=True).cpu().numpy()
    assert np.array_equal(st, R.explore(f, i))
    _assert_equals_ref(b, R, "second")
    assert set(st.tolist()) == {ref.LOST, ref.FULL}   # (scores fall with the frame count, and there is no room for a new cell)
    b.close()


def test_select_against_the_restatement():
    maps, doors = _levels()
    b = _batch(levels=maps + [maps[1]], seed=0xDEADBEEF12345678)
    R = ref.CellArchiveRef(doors + [doors[1]], SLOTS, seed=0xDEADBEEF12345678)
    acts = _acts(21, 12)
    for t in range(12):
        b.step(acts[t])
        f, i = b.dump_state()
        assert np.array_equal(b.archive_explore(status=True).cpu().numpy(), R.explore(f, i))
    # a third level entry no cell was ever stored for (the index outlives npp_assign_levels)
    b.assign_levels(np.array([2, 2], dtype=np.int32), env_ids=np.array([5, 70], dtype=np.int32))
    levels = b.env_levels()
    assert levels[5] == 2 and levels[70] == 2
    rng = np.random.default_rng(22)
    some = rng.integers(0, 2, N).astype(bool)
    masks = [None, torch.ones(N, dtype=torch.uint8, device="cuda"), some, np.zeros(N, dtype=np.uint8), torch.from_numpy(~some).cuda()]
    for c, mask in enumerate(masks):
        got = b.archive_select(mask).cpu().numpy()
        host_mask = None if mask is None else (mask.cpu().numpy() if isinstance(mask, torch.Tensor) else mask)
        before = R.chosen.copy()
        want = R.select(levels, host_mask)
        assert got.dtype == np.int32 and np.array_equal(got, want), (c, np.nonzero(got != want)[0][:8])
        assert got[5] == -1 and got[70] == -1
        if host_mask is not None:
            assert (got[~host_mask.astype(bool)] == -1).all()
        picked = got[got >= 0]
        assert int(R.chosen.sum()) - int(before.sum()) == len(picked)
        _assert_equals_ref(b, R, c)
    assert len(set(got[got >= 0].tolist())) > 2   # the draws spread over the cells
    # the drawn slots restore: every pick is a stored slot of the env's own level
    slots = b.archive_select()
    st = b.archive_restore(torch.arange(N, dtype=torch.int32, device="cuda"), slots, status=True).cpu().numpy()
    assert np.array_equal(st, np.where(np.isin(np.arange(N), [5, 70]), 1, 0))
    b.close()


def _sequence(overlap=0):
    """15 steps with an explore DIRECTLY after every step (nothing that joins or synchronises in between) and a select after every
    fifth; everything the calls produce."""
    b = _batch()
    b.set_step_variant(0)   # (a pinned build: a split step needs no autotuner decision first; same bits)
    if overlap:
        b.set_obs_overlap(overlap)
    acts = _acts(31, 15)
    status, slots = [], []
    for t in range(15):
        b.step(acts[t])
        status.append(b.archive_explore(status=True))
        if t % 5 == 4:
            slots.append(b.archive_select())
    out = {"status": torch.stack(status).cpu().numpy(), "slots": torch.stack(slots).cpu().numpy(), "meta": _meta(b)}
    out.update(_tables(b))
    b.close()
    return out


def _same(a, b):
    for k in ("status", "slots") + TABLES:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["meta"][0].view(np.uint64), b["meta"][0].view(np.uint64)) and np.array_equal(a["meta"][1], b["meta"][1])


def _plain():
    if "plain" not in _cache:
        _cache["plain"] = _sequence()
    return _cache["plain"]


def test_two_handles_agree():
    first = _plain()
    assert first["n_used"][0] > 2 and (first["slots"] >= 0).all()
    _same(first, _sequence())


def test_explore_joins_an_observation_overlap():
    _same(_plain(), _sequence(overlap=40))


def test_refusals_and_life_cycle():
    from nclone_amd import _native as nat

    b = _batch(slots=0)

    def refused(fn, *args, match):
        with pytest.raises(nat.NppError, match=match) as ei:
            fn(*args)
        assert ei.value.code == nat.NPP_ERR_STATE

    refused(b.archive_cells_create, match="no archive")
    refused(b.archive_explore, match="no cell index")
    refused(b.archive_select, match="no cell index")
    refused(b.archive_cells, match="no cell index")
    b.archive_create(SLOTS)
    refused(b.archive_explore, match="no cell index")
    assert b.archive_store([3], [5], status=True).cpu().numpy().tolist() == [0]
    b.archive_cells_create(seed=1)   # empties the archive and owns its slots
    assert not b.archive_meta()["stored"].any()
    assert b.archive_restore([4], [5], status=True).cpu().numpy().tolist() == [3]
    refused(b.archive_store, [3], [5], match="cell index owns the slots")
    assert b.archive_explore(status=True).cpu().numpy()[0] == 0
    assert b.archive_restore([4, 70], [0, 0], status=True).cpu().numpy().tolist() == [0, 2]   # restore works as before
    b.snapshot()
    b.restore()
    refused(b.set_level_pool, [1.0, 1.0], 7, match="checkpoint archive exists")
    # npp_assign_levels keeps the index
    b.assign_levels(np.array([1], dtype=np.int32), env_ids=np.array([10], dtype=np.int32))
    assert b.archive_cells()["n_used"].cpu().numpy()[0] == 2
    assert b.archive_select().cpu().numpy()[10] == 1   # the only cell of level 1
    # enable=False frees the tables and leaves the records
    b.archive_cells_create(enable=False)
    refused(b.archive_select, match="no cell index")
    assert b.archive_meta()["stored"].cpu().numpy().tolist()[:3] == [1, 1, 0]
    assert b.archive_store([3], [5], status=True).cpu().numpy().tolist() == [0]
    # npp_archive_create (any argument) and npp_load_levels drop the index
    b.archive_cells_create()
    b.archive_create(SLOTS)
    refused(b.archive_explore, match="no cell index")
    b.archive_cells_create()
    b.archive_create(0)
    refused(b.archive_cells_create, match="no archive")
    b.archive_create(SLOTS)
    b.archive_cells_create()
    b.load_levels(_levels()[0])
    assert b.archive_num_slots() == 0
    refused(b.archive_explore, match="no cell index")
    # with the pool on there is no archive to index
    b.set_level_pool([1.0, 1.0], 7)
    refused(b.archive_create, SLOTS, match="level pool is on")
    b.close()


def _np(v):
    return v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


@pytest.mark.parametrize("output", ["torch", "numpy"])
def test_vec_env_explore_and_restart_from_archive(output):
    from nclone_amd.vec_env import NppVecEnvironment

    maps, doors = _levels()
    env = NppVecEnvironment(maps, N, level_ids=LEVEL_IDS, output=output, checkpoint_slots=SLOTS, checkpoint_cells=True, checkpoint_seed=9)
    R = ref.CellArchiveRef(doors, SLOTS, seed=9)
    b = env.batch
    env.reset(seed=0)
    acts = _acts(41, 24).cpu().numpy()
    hist, stored = [], {}   # dump rows after every step; slot -> (step, env) of the state it holds
    for t in range(24):
        obs = env.step(acts[t])[0]
        f, i = b.dump_state()
        hist.append((f, i))
        if t < 12:   # (the winners' next 10 steps stay inside the recorded run)
            st = _np(env.archive_explore())
            want = R.explore(f, i)
            assert np.array_equal(st, want)
            for e in np.nonzero(want == 0)[0]:
                stored[int(R.cell_slot[R.keys(f, i)[e]])] = (t, int(e))
    with pytest.raises(RuntimeError, match="cell index owns the slots"):
        env.archive_store(np.full(N, -1, dtype=np.int32))
    done = np.random.default_rng(42).integers(0, 4, N) == 0
    got = env.restart_from_archive(torch.from_numpy(done).cuda() if output == "torch" else done)
    assert set(got) == set(obs)
    slots = env.last_restart_slots.cpu().numpy()
    assert np.array_equal(slots, R.select(LEVEL_IDS, done)) and (slots[done] >= 0).all() and len(set(slots[done].tolist())) > 2
    f, i = b.dump_state()
    for e in range(N):
        if done[e]:
            t0, src = stored[int(slots[e])]
            assert np.array_equal(f[e], hist[t0][0][src]) and np.array_equal(i[e], hist[t0][1][src]), e
        else:   # untouched envs are bit-identical across the call
            assert np.array_equal(f[e], hist[-1][0][e]) and np.array_equal(i[e], hist[-1][1][e]), e
    # the restarted envs are fed their winners' recorded actions: they repeat the winners' future
    replay = _acts(43, 10).cpu().numpy()
    for e in np.nonzero(done)[0]:
        t0, src = stored[int(slots[e])]
        replay[:, e] = acts[t0 + 1:t0 + 11, src]
    for j in range(10):
        env.step(replay[j])
        f, i = b.dump_state()
        for e in np.nonzero(done)[0]:
            t0, src = stored[int(slots[e])]
            assert np.array_equal(f[e], hist[t0 + 1 + j][0][src]) and np.array_equal(i[e], hist[t0 + 1 + j][1][src]), (j, e)
    env.close()
