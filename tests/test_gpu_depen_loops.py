"""The depenetration loop of the register fast path (collide_vs_tiles) exists in two copies per build: one without any arc
code, taken when no lane of the wavefront gathered a circular segment, and the arc-capable one.  These tests drive each
copy on purpose -- and both kinds of lane group inside one wavefront -- and compare the fp64 state and the discrete fields
BIT FOR BIT with the oracle's multiply-square twin, tick by tick (the comparison of test_replays_bit_exact_vs_oracle_mul).

Levels (curriculum-0 set, chosen with the oracle on the CPU):
  * STRAIGHT = 14: its tile array holds none of the ids 10..17 that npp_level.cpp compiles to circular segments;
  * ARCS = 84 (maze:tiny:100007): quarter-circle tiles all around the spawn; under the inputs below the oracle applies
    depenetrations next to a circular tile on about 5 000 of the 19 200 env-ticks;
  * CREASE = 29: the V crease under the spawn, 452 applied depenetrations per 4-tick step at rest (oracle).
No env terminates under these inputs (asserted from the oracle's run), so every tick of every env is compared.

test_table_forms drives the other form of the tile queries, the walk over the level's segment table, with launch
geometries whose candidate registers cannot hold what ARCS and STRAIGHT put around the ninja.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

STRAIGHT, ARCS, CREASE = 14, 84, 29
CIRCULAR_TILE_IDS = tuple(range(10, 18))   # npp_level.cpp: the tile ids that become circular segments
N, TICKS, HOLD, SEED = 16, 1200, 6, 1


@functools.lru_cache(maxsize=None)
def _levels():
    from nclone_amd.levels import curriculum0_levels

    return curriculum0_levels()[0]


def _tiles(level):
    """[44, 25] tile ids incl. the solid border (the layout of Oracle.tiles)."""
    t = np.ones((44, 25), dtype=np.int64)
    t[1:43, 1:24] = np.asarray(_levels()[level][184:184 + 42 * 23]).reshape(23, 42).T
    return t


@functools.lru_cache(maxsize=None)
def _inputs():
    """uint8 [TICKS, N] replay input bytes: a seeded random byte per env, held for HOLD ticks."""
    rng = np.random.default_rng(SEED)
    a = rng.integers(0, 8, size=((TICKS + HOLD - 1) // HOLD, N))
    a = np.repeat(a, HOLD, axis=0)[:TICKS].astype(np.uint8)
    a.setflags(write=False)
    return a


_ORACLE = {}


def _oracle_run(om, level, env):
    """Oracle trajectory of input column `env` on `level`: (f64 [TICKS, 12], i32 [TICKS, 22]); computed once, shared."""
    key = (level, env)
    if key not in _ORACLE:
        o = om.Oracle("mul")
        o.load(_levels()[level])
        F = np.zeros((TICKS, 12), dtype=np.float64)
        D = np.zeros((TICKS, 22), dtype=np.int32)
        for k in range(TICKS):
            h, j = om.controls(int(_inputs()[k, env]))
            o.tick(h, j)
            f, d = o.core()
            F[k], D[k] = f, d[:22]
        assert not np.isin(D[:, 0], (6, 7, 8)).any(), "chosen inputs must keep every env alive and unfinished"
        F.setflags(write=False)
        D.setflags(write=False)
        _ORACLE[key] = (F, D)
    return _ORACLE[key]


_DEVICE = {}


def _device_run(level_of_env, variant, geometry=(16, 4)):
    """Device trajectory of the 16 envs at `geometry` = (lanes per env, wavefronts per workgroup); the default is one
    workgroup of 4 wavefronts with 16 lanes per env.  Dump after every tick.  Cached."""
    key = (tuple(level_of_env), variant, tuple(geometry))
    if key not in _DEVICE:
        from nclone_amd.engine import NppBatch

        ids = sorted(set(level_of_env))
        b = NppBatch(N, autoreset=False)
        b.load_levels([_levels()[i] for i in ids])
        b.set_launch_geometry(*geometry)
        b.set_step_variant(variant)
        b.assign_levels(np.array([ids.index(i) for i in level_of_env], dtype=np.int64))
        d_inputs = torch.from_numpy(np.array(_inputs())).cuda()
        F = np.zeros((TICKS, N, 12), dtype=np.float64)
        D = np.zeros((TICKS, N, 22), dtype=np.int32)
        for k in range(TICKS):
            b.tick(d_inputs[k:k + 1])
            f, di = b.dump_state()
            F[k], D[k] = f, di[:, :22]
        F.setflags(write=False)
        D.setflags(write=False)
        _DEVICE[key] = (F, D)
    return _DEVICE[key]


def _assert_matches_oracle(om, level_of_env, F, D):
    for e, lv in enumerate(level_of_env):
        oF, oD = _oracle_run(om, lv, e)
        bad = np.nonzero((F[:, e] != oF).any(axis=1) | (D[:, e] != oD).any(axis=1))[0]
        if len(bad):
            k = int(bad[0])
            raise AssertionError(("first mismatch", "env", e, "level", lv, "tick", k, F[k, e], oF[k], D[k, e], oD[k]))
        assert np.array_equal(F[:, e].view(np.int64), oF.view(np.int64))   # bits, not values (-0.0, nan)


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_straight_loop_only(variant, oracle_mod):
    """No circular segment exists in the level, so no wavefront can ever take the arc-capable copy of the loop."""
    assert not np.isin(_tiles(STRAIGHT), CIRCULAR_TILE_IDS).any()
    contacts = sum(int((_oracle_run(oracle_mod, STRAIGHT, e)[1][:, 8:10].sum(axis=1) > 0).sum()) for e in range(N))
    assert contacts > 1000, contacts   # the loop applied depenetrations on that many env-ticks (oracle: 2686)
    lv = [STRAIGHT] * N
    F, D = _device_run(lv, variant)
    _assert_matches_oracle(oracle_mod, lv, F, D)


def _arc_contacts(om):
    """env-ticks of the oracle's run on ARCS that applied a depenetration (floor_count + ceiling_count > 0) while the
    ninja's cell or one of its eight neighbours holds a circular tile."""
    circ = np.isin(_tiles(ARCS), CIRCULAR_TILE_IDS)
    hits = 0
    for e in range(N):
        oF, oD = _oracle_run(om, ARCS, e)
        for k in np.nonzero(oD[:, 8] + oD[:, 9] > 0)[0]:
            cx, cy = int(oF[k, 0] // 24), int(oF[k, 1] // 24)
            hits += bool(circ[max(cx - 1, 0):cx + 2, max(cy - 1, 0):cy + 2].any())
    return hits


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_arc_loop(variant, oracle_mod):
    """Circular tiles around the spawn: the wavefronts take the arc-capable copy (precondition from the oracle's own run)."""
    assert _arc_contacts(oracle_mod) > 1000   # oracle: 5038
    lv = [ARCS] * N
    F, D = _device_run(lv, variant)
    _assert_matches_oracle(oracle_mod, lv, F, D)


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_both_kinds_in_one_wavefront(variant, oracle_mod):
    """Levels alternate per env (tables are then read through the caches, not staged per workgroup): every wavefront holds
    two straight-only lane groups beside two that gather arcs, so it runs the arc-capable copy for all four.  Same input
    column per env as above, hence the same bits as the env had in the single-level runs."""
    lv = [STRAIGHT if e % 2 == 0 else ARCS for e in range(N)]
    F, D = _device_run(lv, variant)
    _assert_matches_oracle(oracle_mod, lv, F, D)
    Fs, Ds = _device_run([STRAIGHT] * N, variant)
    Fa, Da = _device_run([ARCS] * N, variant)
    for e in range(N):
        rF, rD = (Fs, Ds) if e % 2 == 0 else (Fa, Da)
        assert np.array_equal(F[:, e].view(np.int64), rF[:, e].view(np.int64)), e
        assert np.array_equal(D[:, e], rD[:, e]), e


def _over_capacity(om, level, capacity):
    """(env-ticks of the oracle's run on `level` whose gather region holds more than `capacity` segments, those of them
    with an applied depenetration).  The region: the cells of the box from the previous to the current position, padded
    by 12.2 px (tick 0 has no previous position in the run and uses its own, a smaller box); segments per cell from the
    level compiler.  Such a tick cannot keep its candidates in registers, so every
    tile query of it walks the table.  (The box ends at the post-collision position where the kernel's ends at the
    pre-collision one; the thresholds below leave a factor of two for cells that flip at a boundary.)"""
    from nclone_amd.engine import compile_level_segments

    rows, _ = compile_level_segments(np.asarray(_levels()[level], dtype=np.float64))
    per_cell = np.zeros((44, 25), dtype=np.int64)
    np.add.at(per_cell, (rows[:, 0].astype(np.int64), rows[:, 1].astype(np.int64)), 1)
    over = applied = 0
    for e in range(N):
        oF, oD = _oracle_run(om, level, e)
        x, y = oF[:, 0], oF[:, 1]
        px, py = np.concatenate([x[:1], x[:-1]]), np.concatenate([y[:1], y[:-1]])
        c0x = np.clip(np.floor((np.minimum(x, px) - 12.2) / 24), 0, 43).astype(np.int64)
        c1x = np.clip(np.floor((np.maximum(x, px) + 12.2) / 24), 0, 43).astype(np.int64)
        c0y = np.clip(np.floor((np.minimum(y, py) - 12.2) / 24), 0, 24).astype(np.int64)
        c1y = np.clip(np.floor((np.maximum(y, py) + 12.2) / 24), 0, 24).astype(np.int64)
        for k in range(TICKS):
            if per_cell[c0x[k]:c1x[k] + 1, c0y[k]:c1y[k] + 1].sum() > capacity:
                over += 1
                applied += bool(oD[k, 8] + oD[k, 9] > 0)
    return over, applied


@pytest.mark.parametrize("level,lanes,least", [(ARCS, 1, 1000), (ARCS, 2, 1000), (STRAIGHT, 1, 300)])
def test_table_forms(level, lanes, least, oracle_mod):
    """1 and 2 lanes per env keep 4 candidate registers per lane (KSlots), 4 and 8 per env: most ticks on ARCS and many on
    STRAIGHT gather more segments than that, and the sweep, the depenetration loop and the wall probe of such a tick all
    take the table form.  Oracle, out of 19 200 env-ticks: ARCS 19 090 over 4 (5 572 with an applied depenetration) and
    10 618 over 8 (2 458); STRAIGHT 1 335 over 4 (582)."""
    over, applied = _over_capacity(oracle_mod, level, lanes * 4)
    print("level %d, %d lanes: %d env-ticks over capacity, %d with an applied depenetration" % (level, lanes, over, applied))
    assert applied >= least, (over, applied)
    lv = [level] * N
    F, D = _device_run(lv, 0, (lanes, 1))
    _assert_matches_oracle(oracle_mod, lv, F, D)


def test_crease_every_variant(oracle_mod):
    """16 envs at rest in the V crease of level 29 (all NOOP): an exact fixed point that runs three substeps of every tick
    to the 32-iteration cap.  Every build gives the oracle's state, and every env reports at least 400 applied
    depenetrations in every step (the oracle applies 452 per 4-tick step there)."""
    from nclone_amd.engine import NppBatch

    o = oracle_mod.Oracle("mul")
    o.load(_levels()[CREASE])
    for _ in range(60):
        o.env_step(0, 4)
    ref, ref_work = [], []
    for _ in range(20):
        w = 0
        for _ in range(4):
            o.tick(0, 0)
            d = o.core()[1]
            w += int(d[8] + d[9])
        ref.append(o.core())
        ref_work.append(w)
    assert min(ref_work) >= 400, ref_work
    acts = torch.zeros(N, dtype=torch.uint8, device="cuda")
    dumps = {}
    for variant in (0, 1, 2):
        b = NppBatch(N, autoreset=False)
        b.load_levels([_levels()[CREASE]])
        b.set_launch_geometry(16, 4)
        b.set_step_variant(variant)
        b.assign_levels(np.zeros(N, dtype=np.int64))
        for _ in range(60):
            b.step(acts, 4)
        work = torch.zeros((20, N), dtype=torch.int16, device="cuda")
        for s in range(20):
            b.step(acts, 4, work_out=work[s])
            f, di = b.dump_state()
            for e in range(N):
                assert np.array_equal(f[e].view(np.int64), ref[s][0].view(np.int64)), (variant, s, e, f[e], ref[s][0])
                assert np.array_equal(di[e, :22], ref[s][1][:22]), (variant, s, e)
        w = work.cpu().numpy()
        print("variant %d: work per step min %d max %d (oracle %d)" % (variant, w.min(), w.max(), ref_work[0]))
        assert w.min() >= 400, (variant, w)
        dumps[variant] = b.dump_state()
    for variant in (1, 2):
        assert np.array_equal(dumps[variant][0].view(np.int64), dumps[0][0].view(np.int64))
        assert np.array_equal(dumps[variant][1], dumps[0][1])
