"""The step kernel on injected ninja states (tests/inject_states.py): every row of the table is one env of ONE NppBatch; reset,
NppBatch.set_ninja_state, then TICKS single ticks with a state dump after each.  The fp64 state and the discrete fields are compared BIT
FOR BIT with the oracle's multiply-square twin (int64 view of the 12 doubles, first 22 discrete columns), every tick up to and including
the one that leaves the env terminal (state 6, 7 or 8).  (Both twins share one known deviation from the reference, the sign of a zero
yspeed after a flat landing: DESIGN.md 2.1; against the reference's fixture the doubles are compared by value, as everywhere on the GPU.)

Rollouts never reach most of these rows: sweep boxes of four and more columns (cand_gather's veto), region walks over many columns at
every lane count, the 32-iteration cap from deep inside a solid, the reference's three hard-coded positions, the 1e-16 exit, the wall
probe's 10.1 px radius and 1e-5 gate to the ulp, query boxes that touch a cell bound exactly (tests/test_inject_host.py asserts that
the rows do get there).

One case is one launch geometry (lanes per env, wavefronts per workgroup, build variant) in one env order: `grouped` keeps the envs of a
level together, so workgroups stage their level's tables in LDS; `interleaved` alternates the levels env by env, so the tables are read
through the caches.  Every case must give the oracle's bits, hence the same bits as every other; each case is also compared with the first
one that ran.  The oracle's run is computed once and shared.
"""
import numpy as np
import pytest

from tests import inject_states as gen

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

POS_TOL = 1e-5   # tests/test_gpu_parity.py: the north-star tolerance on positions against the reference's fixture
GEOMETRIES = [(1, 1, 0), (2, 2, 0), (4, 4, 0), (8, 4, 0), (32, 2, 0), (64, 1, 0), (16, 4, 0), (16, 4, 1), (16, 4, 2)]
ORDERS = ("grouped", "interleaved")


def _order(name):
    """env -> row of the table.  grouped: the table's own order (rows are sorted by level), each level's block filled up to a
    multiple of 64 envs with repeats of its first rows -- a workgroup holds at most 64 envs, and the level tables are staged in LDS only
    when no workgroup of the launch mixes levels; interleaved: round robin over the levels until the shorter ones run out."""
    level = gen.states()[0]
    if name == "grouped":
        blocks = []
        for lv in range(len(gen.LEVEL_IDS)):
            rows = np.nonzero(level == lv)[0]
            blocks.append(np.concatenate([rows, rows[:-len(rows) % 64]]))
        return np.concatenate(blocks)
    rank = np.zeros(len(level), dtype=np.int64)
    for lv in range(len(gen.LEVEL_IDS)):
        m = level == lv
        rank[m] = np.arange(m.sum())
    return np.lexsort((level, rank))


_DEVICE = {}   # the runs later tests need again: the first one of the session and FIXTURE_RUN (40 MB each, so not all 18)
FIXTURE_RUN = ((16, 4, 0), "grouped")


def _device_run(geometry, order):
    """(F f64 [n, TICKS, 12], D i32 [n, TICKS, 22]) in table row order."""
    key = (tuple(geometry), order)
    if key not in _DEVICE:
        from nclone_amd.engine import NppBatch

        level, xyv, _, _ = gen.states()
        perm = _order(order)
        n = len(level)
        lanes, waves, variant = geometry
        b = NppBatch(len(perm), autoreset=False)
        b.load_levels(list(gen.level_maps()))
        b.set_launch_geometry(lanes, waves)
        b.set_step_variant(variant)
        b.assign_levels(level[perm].astype(np.int64))
        b.reset()
        b.set_ninja_state(xyv[perm])
        d_inputs = torch.from_numpy(np.ascontiguousarray(gen.inputs()[:, perm])).cuda()
        F = np.zeros((n, gen.TICKS, 12), dtype=np.float64)
        D = np.zeros((n, gen.TICKS, 22), dtype=np.int32)
        for t in range(gen.TICKS):
            b.tick(d_inputs[t:t + 1])
            f, di = b.dump_state()
            F[perm, t], D[perm, t] = f, di[:, :22]
        assert b.launch_geometry() == (lanes, waves) and b.step_variant()[0] == variant
        b.close()
        F.setflags(write=False)
        D.setflags(write=False)
        if _DEVICE and key != FIXTURE_RUN:
            return F, D
        _DEVICE[key] = (F, D)
    return _DEVICE[key]


def _first_mismatch(bad, F, D, oF, oD):
    level, xyv, family, _ = gen.states()
    k, t = (int(v) for v in np.argwhere(bad)[0])
    return ("first of %d mismatching env-ticks" % int(bad.sum()), "row", k, "family", gen.FAMILY_NAMES[family[k]], "level", int(level[k]),
            "tick", t, "injected", xyv[k].tolist(), "device", F[k, t].tolist(), "expected", oF[k, t].tolist(), D[k, t].tolist(), oD[k, t].tolist())


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "g%dw%dv%d" % g)
def test_injected_states_bit_exact(geometry, order, oracle_mod):
    oF, oD, valid = gen.oracle_run(oracle_mod, "mul")
    first = next(iter(_DEVICE.values()), None)
    F, D = _device_run(geometry, order)
    bad = valid & ((F.view(np.int64) != oF.view(np.int64)).any(axis=2) | (D != oD).any(axis=2))   # bits, not values (-0.0)
    if bad.any():
        raise AssertionError(_first_mismatch(bad, F, D, oF, oD))
    if first is not None:
        assert np.array_equal(F.view(np.int64)[valid], first[0].view(np.int64)[valid])
        assert np.array_equal(D[valid], first[1][valid])


def test_injected_states_vs_reference_fixture(golden):
    """the reference's own run of the fixture's subset of the rows: discrete rows identical, the four doubles within POS_TOL (the
    device squares by multiplication, the reference by pow)"""
    z = golden.z("inject")
    idx = z["idx"]
    assert np.array_equal(np.ascontiguousarray(gen.states()[1][idx]).view(np.uint64), z["xyv"])
    F, D = _device_run(*FIXTURE_RUN)
    live = np.arange(gen.TICKS)[None, :] < z["nt"].astype(np.int64)[:, None]
    ref = z["t"].view(np.float64)
    err = np.abs(F[idx][:, :, :4] - ref)[live]
    print("max |device - reference| over %d state-ticks: %.3g" % (int(live.sum()), err.max()))
    bad = live & ((np.abs(F[idx][:, :, :4] - ref) > POS_TOL).any(axis=2) | (D[idx][:, :, :20].clip(0, 255) != z["d"]).any(axis=2))
    assert not bad.any(), ("first of %d" % bad.sum(), idx[np.argwhere(bad)[0][0]], np.argwhere(bad)[0])


def test_set_ninja_state_writes_four_planes_only():
    """the hook itself: the four planes of the named envs and nothing else; a non-finite value is refused and nothing is written"""
    from nclone_amd.engine import NppBatch

    n = 64
    b = NppBatch(n, autoreset=False)
    b.load_levels([gen.level_maps()[gen.STRAIGHT]])
    b.assign_levels(np.zeros(n, dtype=np.int64))
    acts = torch.full((n,), 2, dtype=torch.uint8, device="cuda")
    for _ in range(5):
        b.step(acts, 4)   # some history in the other planes and words
    f0, i0 = b.dump_state()
    cs0 = b.entity_checksum()
    xyv = np.column_stack([np.linspace(100, 900, 20), np.linspace(50, 500, 20), np.full(20, -3.25), np.full(20, -0.0)])
    b.set_ninja_state(xyv, env0=7)
    f1, i1 = b.dump_state()
    assert np.array_equal(f1[7:27, :4].view(np.int64), xyv.view(np.int64))   # bits: the -0.0 column too
    keep = np.ones(n, dtype=bool)
    keep[7:27] = False
    assert np.array_equal(f1[keep].view(np.int64), f0[keep].view(np.int64))
    assert np.array_equal(f1[:, 4:].view(np.int64), f0[:, 4:].view(np.int64))
    assert np.array_equal(i1, i0) and np.array_equal(b.entity_checksum(), cs0)
    for bad in (np.nan, np.inf, -np.inf):
        x = xyv.copy()
        x[13, 2] = bad
        with pytest.raises(ValueError):
            b.set_ninja_state(x, env0=7)
        f2, i2 = b.dump_state()
        assert np.array_equal(f2.view(np.int64), f1.view(np.int64)) and np.array_equal(i2, i1)
    with pytest.raises(ValueError):
        b.set_ninja_state(xyv, env0=n - 10)   # runs past the last env
    with pytest.raises(ValueError):
        b.set_ninja_state(xyv[:, :3])
    b.close()
