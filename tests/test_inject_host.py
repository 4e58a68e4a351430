"""The CPU oracle on injected ninja states (tests/inject_states.py): positions inside solids, speeds of many cells per tick,
lattice points to the ulp, the reference's three hard-coded positions, every segment junction of a map that shows every tile.

test_oracle_matches_reference compares the oracle ("pow": squares like CPython) with the reference's own run of a subset of the rows
(tests/golden/inject.npz, written by tests/golden/make_golden_inject.py): the four doubles BY BITS, zero signs included, the discrete row
identical, every tick up to and including the one that leaves the ninja terminal.  One exception, a known deviation of both twins
(DESIGN.md "injected states"): a zero yspeed is compared without its sign.

The census tests assert from the oracle's run of ALL rows that the rows do what they are for.  Each threshold is about half of what the
oracle gives on this table (the measured figure stands beside it); the two lattice thresholds are fixed at 50.
"""
import numpy as np
import pytest

from tests import inject_states as gen


@pytest.fixture(scope="module")
def run(oracle_mod):
    from nclone_amd import build_native

    build_native.build()   # the generator reads compiled segment tables (host-only entry of the native library)
    return gen.oracle_run(oracle_mod, "pow")


def _sel(level, family):
    lv, _, fam, _ = gen.states()
    return (lv == level) & np.isin(fam, family)


def _work(run):
    """applied depenetrations of the first tick (floor_count + ceiling_count: both are cleared at the start of a tick)"""
    return run[1][:, 0, 8] + run[1][:, 0, 9]


def test_table_is_deterministic_and_in_range():
    level, xyv, family, group = gen.states()
    assert np.isfinite(xyv).all() and len(level) == len(xyv) == len(family) == len(group) == gen.inputs().shape[1]
    free = np.isin(family, (gen.FREE, gen.FAST12, gen.FAST45))
    assert (xyv[free, 0] >= 24).all() and (xyv[free, 0] <= 1032).all() and (xyv[free, 1] >= 24).all() and (xyv[free, 1] <= 576).all()
    assert (np.hypot(xyv[:, 2], xyv[:, 3]) <= gen.V_MAX * (1 + 1e-12)).all()
    for lv in range(len(gen.LEVEL_IDS)):
        for f in (gen.FREE, gen.FAST12, gen.FAST45, gen.LATTICE):
            assert _sel(lv, f).sum() > 0
    assert _sel(gen.SYNTH, gen.BANDAID).sum() == 9 and _sel(gen.SYNTH, gen.CORNERS).sum() > 0
    # every ulp-neighbour group: 5 rows, 5 distinct positions within 4 ulp of each other
    lat = family == gen.LATTICE
    g, counts = np.unique(group[lat], return_counts=True)
    assert (counts == 5).all() and (group[~lat] == -1).all()
    tiles = gen.tile_grid(gen.level_maps()[gen.SYNTH])
    assert sorted(np.unique(tiles[1:43, 1:24]).tolist()) == list(range(34))   # every tile id the level compiler accepts
    for t, (cx, cy) in gen.exhibit_cells().items():
        around = tiles[cx - 1:cx + 2, cy - 1:cy + 2].copy()
        assert around[1, 1] == t
        around[1, 1] = 0
        assert not around.any(), t   # empty neighbours on all sides


def test_oracle_matches_reference(run, golden):
    z = golden.z("inject")
    idx = z["idx"]
    _, xyv, _, _ = gen.states()
    assert np.array_equal(np.ascontiguousarray(xyv[idx]).view(np.uint64), z["xyv"]), "the generator's table moved: regenerate inject.npz"
    lv, _, fam, _ = gen.states()
    assert np.array_equal(lv[idx], z["level"]) and np.array_equal(fam[idx], z["family"])
    pairs = set(zip(z["level"].tolist(), z["family"].tolist()))
    for level in range(len(gen.LEVEL_IDS)):
        for f in (gen.FREE, gen.FAST12, gen.FAST45, gen.LATTICE):
            assert (level, f) in pairs
    assert (gen.SYNTH, gen.BANDAID) in pairs and (gen.SYNTH, gen.CORNERS) in pairs
    F, D, valid = run
    nt = z["nt"].astype(np.int64)
    # the fixture stops after the terminal tick; the oracle's `valid` marks the same ticks
    assert np.array_equal(valid[idx].sum(axis=1), nt)
    live = np.arange(gen.TICKS)[None, :] < nt[:, None]
    got_bits = np.ascontiguousarray(F[idx][:, :, :4]).view(np.uint64)
    differ = got_bits != z["t"]
    # yspeed, and only yspeed, is compared without the sign of a zero.  ninja.py:313-318 (:316 in the issue's count) sets dx to the
    # INTEGER 0 when abs(dx) <= 1e-7; -dx is then 0 and yspeed = cross_product * inv_dist_sq * (-dx) a zero with cross_product's sign,
    # where the oracle and the HIP kernel negate a floating zero and get the other sign -- on every landing on a flat floor.  Making
    # the kernel's zero the reference's (0.0 - ddx) costs the depenetration loop one fp64 add per iteration, 0.6 % of the doors
    # workload, so both twins keep the flaw (DESIGN.md "injected states").  With 0.0 - dx in the oracle this comparison passed by bits.
    vy_zero_sign = differ[:, :, 3] & (F[idx][:, :, 3] == 0) & (z["t"][:, :, 3].view(np.float64) == 0)
    differ[:, :, 3] &= ~vy_zero_sign
    print("state-ticks whose zero yspeed has the other sign: %d of %d (in %d of %d states)"
          % (int((vy_zero_sign & live).sum()), int(live.sum()), int((vy_zero_sign & live).any(axis=1).sum()), len(idx)))
    bad = live & (differ.any(axis=2) | (D[idx][:, :, :20].clip(0, 255) != z["d"]).any(axis=2))
    if bad.any():
        r, t = np.argwhere(bad)[0]
        raise AssertionError(("first of %d mismatching state-ticks" % bad.sum(), "row", int(idx[r]), "family", gen.FAMILY_NAMES[fam[idx[r]]],
                              "level", int(lv[idx[r]]), "tick", int(t), "injected", xyv[idx[r]].tolist(),
                              "oracle", F[idx[r], t, :4].tolist(), "reference", z["t"][r, t].view(np.float64).tolist(),
                              D[idx[r], t, :20].tolist(), z["d"][r, t].tolist()))


def test_census_depenetration_cap(run):
    """first ticks that run the depenetration loops to 32 applied steps and more (the cap of one pass; four passes per tick)"""
    w = _work(run)
    uniform = (gen.FREE, gen.FAST12, gen.FAST45)
    arcs, crease, straight = int((w[_sel(gen.ARCS, uniform)] >= 32).sum()), int((w[_sel(gen.CREASE, uniform)] >= 32).sum()), \
        int((w[_sel(gen.STRAIGHT, uniform)] >= 4).sum())
    print("first tick: >= 32 applied on level 84: %d, on level 29: %d; >= 4 on level 14: %d (of 3000 uniform rows each)" % (arcs, crease, straight))
    assert arcs >= 500       # oracle: 1022
    assert crease >= 70      # oracle: 138
    assert straight >= 210   # oracle: 428


def test_census_many_columns(run):
    """|vx| > 26: the sweep box spans four or more columns, which cand_gather's registers refuse"""
    _, xyv, _, _ = gen.states()
    n = [int((np.abs(xyv[_sel(lv, gen.FAST45), 2]) > 26).sum()) for lv in range(len(gen.LEVEL_IDS))]
    print("fast45 rows with |vx| > 26 per level:", n)
    assert min(n) >= 200     # this table: 397, 421, 434, 413 of 750


def test_census_lattice_thresholds(run):
    """ulp-neighbour groups inside which a first-tick outcome takes both values: the rows do straddle the thresholds"""
    _, _, family, group = gen.states()
    lat = family == gen.LATTICE
    g = group[lat]
    n = np.bincount(g)
    walled = np.bincount(g, weights=run[1][lat, 0, 2])
    contact = np.bincount(g, weights=(_work(run)[lat] > 0))
    both_walled = int(((walled > 0) & (walled < n)).sum())
    both_contact = int(((contact > 0) & (contact < n)).sum())
    print("lattice groups: %d; walled takes both values in %d, floor_count + ceiling_count is 0 and > 0 in %d" % (len(n), both_walled, both_contact))
    assert both_walled >= 50    # oracle: 99
    assert both_contact >= 50   # oracle: 70


def test_census_band_aid(run):
    """all 9 band-aid rows land in the branch's loop: the closest point lies straight below, one applied depenetration, and the
    ninja is put back on the floor with x untouched"""
    m = _sel(gen.SYNTH, gen.BANDAID)
    _, xyv, _, _ = gen.states()
    assert m.sum() == 9 and (_work(run)[m] >= 1).all()
    assert np.array_equal(run[0][m, 0, 0], xyv[m, 0])


def _dist_to_segments(px, py, rows):
    """[n, m] distance from n points to m rows of a compiled segment table (linear: point-segment; arc: to the quarter circle)."""
    r = rows.astype(np.float64)
    px, py = px[:, None], py[:, None]
    x1, y1, x2, y2 = r[:, 3], r[:, 4], r[:, 5], r[:, 6]
    wx, wy = x2 - x1, y2 - y1
    l2 = np.where(rows[:, 2] == 0, wx * wx + wy * wy, 1.0)
    u = np.clip(((px - x1) * wx + (py - y1) * wy) / l2, 0, 1)
    lin = np.hypot(px - (x1 + u * wx), py - (y1 + u * wy))
    # arc rows: x1, y1 centre; x2, y2 = hor, ver (+-1)
    dx, dy = px - x1, py - y1
    inq = (dx * x2 > 0) & (dy * y2 > 0)
    ends = np.minimum(np.hypot(px - (x1 + 24 * x2), py - y1), np.hypot(px - x1, py - (y1 + 24 * y2)))
    arc = np.where(inq, np.abs(np.hypot(dx, dy) - 24.0), ends)
    return np.where(rows[:, 2] == 0, lin, arc)


def test_census_every_tile_id(run):
    """every tile id 1..33 (0 has no segment) has a row whose closest segment at the first tick is one of that tile's: the row
    stands within 9 px of a segment of the tile's cell -- every other cell's segments are then more than 14 px away, since the cells
    around an exhibited tile are empty -- at under 1 px per tick, and the oracle applied a depenetration in that tick"""
    from nclone_amd.engine import compile_level_segments

    rows, _ = compile_level_segments(gen.level_maps()[gen.SYNTH])
    lv, xyv, _, _ = gen.states()
    m = (lv == gen.SYNTH) & (np.hypot(xyv[:, 2], xyv[:, 3]) < 1.0) & (_work(run) > 0)
    px, py = xyv[m, 0], xyv[m, 1]
    hits = {}
    for t, (cx, cy) in gen.exhibit_cells().items():
        own = rows[(rows[:, 0] == cx) & (rows[:, 1] == cy)]
        assert len(own) > 0, t
        near = (np.abs(px - (24 * cx + 12)) < 24) & (np.abs(py - (24 * cy + 12)) < 24)
        hits[t] = int((_dist_to_segments(px[near], py[near], own).min(axis=1) < 9.0).sum())
    print("rows per tile id whose first-tick closest segment is the tile's:", hits)
    assert min(hits.values()) >= 48, hits   # oracle: 96 (tile 7) .. 311 (tile 1)
