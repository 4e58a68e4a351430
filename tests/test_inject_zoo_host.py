"""The CPU oracle on injected ninja and mover states at the entity code's thresholds (tests/inject_zoo_states.py).

test_oracle_matches_reference compares the oracle ("pow": squares like CPython) with the reference's own run of a subset of the rows
(tests/golden/inject_zoo.npz, written by tests/golden/make_golden_inject_zoo.py): the ninja's four doubles BY BITS, the discrete row
identical, every mover's four doubles BY BITS (the death balls' too: the pow oracle calls the same libm), the entity checksum
within ENT_TOL, every tick up to and including the one that leaves the ninja terminal.  One exception, the known deviation of both
twins: a zero yspeed is compared without its sign.

The census tests assert from the oracle's run of ALL rows that the rows get where they are meant to go.  For a threshold, the count is
the number of ulp-neighbour groups (5 rows, -2..2 ulp apart in one coordinate, same inputs) inside which the outcome of the tick the
threshold decides takes both values; the outcome is everything discrete the tick leaves behind -- the 22 discrete columns (state,
counts, walled, gold, doors ...), the checksum's state code and active count, the per-entity states -- since inside a group nothing
else can flip it.  Each bar is about half of what the oracle gives on this table; the measured figure stands beside it.
"""
import numpy as np
import pytest

from tests import inject_zoo_states as gen

ENT_TOL = 1e-9   # tests/test_gpu_zoo.py: the project's bar on entity checksums


@pytest.fixture(scope="module")
def run(oracle_mod):
    from nclone_amd import build_native

    build_native.build()   # the generator reads compiled level tables (host-only entries of the native library)
    return gen.oracle_run(oracle_mod, "pow")


def _sel(level, family):
    s = gen.states()
    return (s["level"] == level) & np.isin(s["family"], family)


def test_table_is_deterministic_and_in_range(oracle_mod):
    from nclone_amd import build_native
    from nclone_amd.engine import compile_level_zoo

    build_native.build()
    s = gen.states()
    n = len(s["level"])
    assert all(len(a) == n for a in s.values()) and gen.inputs().shape == (gen.TICKS, n)
    again = gen.states.__wrapped__()   # a second generation, past the cache: the same table to the bit
    assert all(np.array_equal(np.ascontiguousarray(s[k]).view(np.uint8), np.ascontiguousarray(again[k]).view(np.uint8)) for k in s)
    assert np.array_equal(gen.inputs(), gen.inputs.__wrapped__())
    assert np.isfinite(s["xyv"]).all() and (np.hypot(s["xyv"][:, 2], s["xyv"][:, 3]) <= gen.V_MAX * (1 + 1e-12)).all()
    assert (np.diff(s["level"]) >= 0).all()   # rows are ordered by level
    # ulp-neighbour groups: 5 rows each, one level, one threshold, the same input bytes, positions within 4 ulp
    g = s["group"]
    grouped = g >= 0
    ids, start, counts = np.unique(g[grouped], return_index=True, return_counts=True)
    assert (counts == 5).all()
    rows = np.nonzero(grouped)[0]
    assert np.array_equal(g[rows].reshape(-1, 5), np.repeat(ids, 5).reshape(-1, 5))   # a group's rows are consecutive
    for col in ("level", "thr", "family"):
        assert (np.ptp(s[col][rows].reshape(-1, 5), axis=1) == 0).all()
    assert (np.ptp(gen.inputs()[:, rows].reshape(gen.TICKS, -1, 5), axis=2) == 0).all()
    moved = (np.ptp(s["xyv"][rows].reshape(-1, 5, 4), axis=1) > 0).sum(axis=1) + (np.ptp(s["mxyab"][rows].reshape(-1, 5, 8), axis=1) > 0).sum(axis=1)
    assert (moved == 1).all()   # exactly one coordinate walks
    # the levels hold what the families aim at, where they aim
    for lv in (gen.PLAIN, gen.STATIC, gen.MOVERS, gen.BALLS):
        o = oracle_mod.Oracle("pow")
        assert o.load(gen.level_maps()[lv]) == 0
        got = sorted((int(r[1]), r[2], r[3]) for r in o.dump_entities())
        assert got == sorted((t, x, y) for t, x, y, _ in gen.entities(lv)), lv
        mv = o.dump_movers()
        assert [(k, x, y) for k, _, x, y, _ in gen.movers(lv)] == [(k, r[0], r[1]) for k, r in enumerate(mv)], lv
        cells = [(int(r[4]), int(r[5])) for r in o.dump_entities()] + [(21, 16)]
        for i, a in enumerate(cells):   # 3 x 3 neighbourhoods do not touch (two boost pads share a cell on purpose; PLAIN's exit pair)
            for b in cells[i + 1:]:
                assert a == b or max(abs(a[0] - b[0]), abs(a[1] - b[1])) >= 3 or (lv == gen.PLAIN and {a, b} == {(30, 20), (29, 20)}), (lv, a, b)
        if lv == gen.MOVERS:   # the rings around the drones stand around where their first move takes them
            o.tick(0, 0)
            after = {int(k): (r[0], r[1]) for k, r in enumerate(o.dump_movers())}
            for k, t, x, y, _ in gen.movers(lv):
                if t == 14:
                    assert after[k] == (x + 8.0 / 7, y)
                if t == 26:
                    assert after[k] == (x, y + 1.3)
    # PLAIN selects the plain kernels: no mover, no door counter, none of the zoo's kinds
    assert len(compile_level_zoo(gen.level_maps()[gen.PLAIN])[2]) == 0
    assert {e[0] for e in gen.level_specs()[gen.PLAIN]} <= {1, 2, 6, 21}
    for lv, fams in ((gen.PLAIN, (gen.RING, gen.FREE, gen.FAST)), (gen.STATIC, (gen.RING, gen.ONEWAY, gen.PAD, gen.FREE, gen.FAST)),
                     (gen.MOVERS, tuple(f for f in range(len(gen.FAMILY_NAMES)) if f not in (gen.ONEWAY, gen.PAD, gen.BALL_PAIR))),
                     (gen.BALLS, (gen.RING, gen.FREE, gen.FAST, gen.BALL_FREE, gen.BALL_FAST, gen.BALL_PAIR)),
                     (gen.REAL, (gen.FREE, gen.FAST, gen.BALL_FREE, gen.BALL_FAST))):
        for f in fams:
            assert _sel(lv, f).sum() > 0, (lv, f)
    assert s["fresh"].sum() == _sel(gen.BALLS, gen.BALL_PAIR).sum() > 0
    # no ninja on a ball's centre (the reference divides by that distance)
    balls = s["mslot"][:, 0] >= 0
    assert (np.hypot(s["xyv"][balls, 0] - s["mxyab"][balls, 0, 0], s["xyv"][balls, 1] - s["mxyab"][balls, 0, 1]) > 0).all()


def test_oracle_matches_reference(run, golden):
    z = golden.z("inject_zoo")
    s = gen.states()
    idx = z["idx"]
    assert np.array_equal(idx, gen.golden_subset())
    moved = "the generator's table moved: regenerate inject_zoo.npz"
    assert np.array_equal(np.ascontiguousarray(s["xyv"][idx]).view(np.uint64), z["xyv"]), moved
    assert np.array_equal(np.ascontiguousarray(s["mxyab"][idx]).view(np.uint64), z["mxyab"]), moved
    assert np.array_equal(s["mslot"][idx], z["mslot"]) and np.array_equal(s["mfield"][idx], z["mfield"]), moved
    assert np.array_equal(s["level"][idx], z["level"]) and np.array_equal(s["family"][idx], z["family"])
    have = set(zip(z["level"].tolist(), z["family"].tolist()))
    assert have == set(zip(s["level"].tolist(), s["family"].tolist()))   # every (level, family) pair of the table
    g = s["group"]
    picked = np.zeros(len(g), dtype=bool)
    picked[idx] = True
    assert (np.bincount(g[picked & (g >= 0)], minlength=g.max() + 1) % 5 == 0).all()   # whole ulp groups only
    F, D, C, M, valid = run["F"], run["D"], run["C"], run["M"], run["valid"]
    nt = z["nt"].astype(np.int64)
    assert np.array_equal(valid[idx].sum(axis=1), nt)   # the fixture stops after the terminal tick; `valid` marks the same ticks
    live = np.arange(gen.TICKS)[None, :] < nt[:, None]
    differ = np.ascontiguousarray(F[idx][:, :, :4]).view(np.uint64) != z["t"]
    # the one exemption: yspeed, and only yspeed, without the sign of a zero
    vy_zero_sign = differ[:, :, 3] & (F[idx][:, :, 3] == 0) & (z["t"][:, :, 3].view(np.float64) == 0)
    differ[:, :, 3] &= ~vy_zero_sign
    movers = np.nan_to_num(M[idx][:, :, :, :4], nan=0.0)   # NaN marks "past the level's movers"; the fixture has 0 there
    bad = {"ninja": differ.any(axis=2), "discrete": (D[idx][:, :, :20].clip(0, 255) != z["d"]).any(axis=2),
           "checksum": (np.abs(C[idx] - z["e"]) > ENT_TOL).any(axis=2),
           "movers": (np.ascontiguousarray(movers).view(np.uint64) != z["m"]).any(axis=(2, 3))}
    print("state-ticks %d in %d states; zero yspeed with the other sign: %d" % (int(live.sum()), len(idx), int((vy_zero_sign & live).sum())))
    for what, b in bad.items():
        b = b & live
        if b.any():
            r, t = (int(v) for v in np.argwhere(b)[0])
            k = int(idx[r])
            raise AssertionError((what, "first of %d mismatching state-ticks" % b.sum(), "row", k, gen.LEVEL_NAMES[s["level"][k]],
                                  gen.FAMILY_NAMES[s["family"][k]], "tick", t, "injected", s["xyv"][k].tolist(), s["mslot"][k].tolist(),
                                  s["mxyab"][k].tolist(), s["mfield"][k].tolist(), "oracle", F[k, t, :4].tolist(), D[k, t, :20].tolist(),
                                  C[k, t].tolist(), movers[r, t].tolist(), "reference", z["t"][r, t].view(np.float64).tolist(),
                                  z["d"][r, t].tolist(), z["e"][r, t].tolist(), z["m"][r, t].view(np.float64).tolist()))


def _outcome(run, rows, tick):
    return np.concatenate([run["D"][rows, tick], run["C"][rows, tick, 4:6].astype(np.int64), run["E"][rows, tick]], axis=1)


def straddling_groups(run, name):
    """(groups of the threshold, groups inside which the outcome of the threshold's tick takes both values)"""
    s = gen.states()
    ti = gen.THR[name]
    rows = np.nonzero((s["thr"] == ti) & (s["group"] >= 0))[0]
    out = _outcome(run, rows, gen.THRESHOLDS[ti][2]).reshape(len(rows) // 5, 5, -1)
    return len(out), int((out != out[:, :1]).any(axis=(1, 2)).sum())


# threshold -> (bar, the oracle's count on this table, groups).  Only the d = 0 groups can straddle (a fifth of all), and of
# those the ones whose walked coordinate moves the compared quantity by more than its rounding error.
CENSUS = {
    "mine_toggle_13.5": (7, 14, 80), "mine_untoggle_14.5": (7, 14, 80), "mine_kill_14": (7, 14, 80), "gold_16": (7, 14, 80),
    "exit_door_22": (4, 8, 80), "exit_switch_16": (7, 14, 80), "locked_switch_15": (7, 14, 80), "regular_door_20": (7, 14, 80),
    "trap_switch_15": (7, 14, 80), "launch_16": (39, 78, 640), "boost_16": (14, 28, 160), "zap_17.5": (7, 14, 80), "mini_14": (7, 14, 80),
    "ball_15": (21, 42, 240), "bounce_19": (40, 80, 160), "bounce_19.1": (17, 34, 160), "thwump_19": (40, 80, 400),
    "thwump_19.1": (23, 46, 400), "shove_22": (10, 20, 100), "shove_22.1": (10, 20, 100), "square_diagonal": (36, 72, 72),
    "thwump_strip_12": (8, 16, 80), "oneway_lateral_17.1": (66, 133, 320), "oneway_lateral_21.1": (25, 50, 320),
    "oneway_normal_0": (39, 79, 240), "oneway_normal_10": (38, 76, 240), "oneway_old_8.9": (38, 76, 480),
    "launch_plane_10.1": (24, 48, 400), "lane_38": (8, 16, 80), "lane_cell": (12, 24, 72), "shove_launch_0.2": (4, 8, 40),
}


@pytest.mark.parametrize("name", [t[0] for t in gen.THRESHOLDS if t[0] != "boost_speed_0"])
def test_census_threshold(run, name):
    """ulp-neighbour groups inside which the threshold's outcome takes both values: the rows do straddle it"""
    bar, measured, groups = CENSUS[name]
    n, both = straddling_groups(run, name)
    print("%s (%s): %d groups, the outcome takes both values in %d (recorded: %d)" % (name, gen.THRESHOLDS[gen.THR[name]][1], n, both, measured))
    assert n == groups and both >= bar > 0


def test_census_boost_speed_zero(run, oracle_mod):
    """the boost pads' vel_norm > 0 gate (entity_boost_pad.py:56) is decided by the injected speed, which no ulp walk of the position
    changes: rows that touch a pad with a speed whose norm is 0 -- zeros of both signs, a denormal, squares that underflow -- keep their
    speed; the others gain 2 px per tick per pad, and rows between the pads touch both in the same tick.  "Keep" is judged against the
    same row on the PLAIN level, which has nothing there."""
    s = gen.states()
    rows = np.nonzero(s["thr"] == gen.THR["boost_speed_0"])[0]
    vx, vy = s["xyv"][rows, 2], s["xyv"][rows, 3]
    zero = np.sqrt(vx * vx + vy * vy) == 0
    touching = np.round(run["C"][rows, 0, 4] / 13).astype(int)   # the checksum's code: 13 per touching pad, nothing else on this level moves it
    assert (touching >= 1).all()
    o = oracle_mod.Oracle("pow")
    o.load(gen.level_maps()[gen.PLAIN])
    plain = np.zeros((len(rows), 4))
    for i, k in enumerate(rows):
        o.reset()
        o.set_ninja(*s["xyv"][k])
        o.tick(*oracle_mod.controls(int(gen.inputs()[0, k])))
        plain[i] = o.core()[0][:4]
    kept = (run["F"][rows, 0, :4] == plain).all(axis=1)
    print("boost rows %d: norm 0 and speed kept %d, boosted %d, touching both pads %d" % (len(rows), int((zero & kept).sum()), int((~zero & ~kept).sum()),
                                                                                        int((touching == 2).sum())))
    assert np.array_equal(zero, kept)
    assert (zero & kept).sum() >= 60        # oracle: 125
    assert (~zero & ~kept).sum() >= 25      # oracle: 50
    assert (touching == 2).sum() >= 70      # oracle: 140


def test_census_ball_branches(run):
    """death ball rows per branch of ball_think, counted by the oracle's debug counters over all ticks (the sweep box from the
    injected speed): the register-to-table fall-back needs a sweep box of four or more cell columns, |vx| > 26"""
    s = gen.states()
    fams = (gen.BALL_FREE, gen.BALL_FAST, gen.BALL_LATTICE, gen.BALL_SPEED)
    rows = np.isin(s["family"], fams)
    wide = int((np.abs(s["mxyab"][rows][:, :, 2]).max(axis=1) > 26).sum())
    hit = (run["B"][rows] > 0).any(axis=1).sum(axis=0)
    print("ball rows %d: sweep box of >= 4 columns %d; rows with >= 16 applied depenetrations %d, dist == 0 bail %d, bounce_strength 2 %d, "
          "speed snap %d" % (int(rows.sum()), wide, *hit))
    assert wide >= 100        # this table: 216
    assert hit[0] >= 170      # oracle: 349
    assert hit[1] >= 530      # oracle: 1076
    assert hit[2] >= 390      # oracle: 790
    assert hit[3] >= 110      # oracle: 227
    speed = s["family"] == gen.BALL_SPEED
    first = run["B"][speed, 0]
    print("ball_speed rows %d: first tick bounce_strength 2 in %d, snap in %d" % (int(speed.sum()), int((first[:, 2] > 0).sum()), int((first[:, 3] > 0).sum())))
    assert 30 <= (first[:, 2] > 0).sum() < speed.sum() and 65 <= (first[:, 3] > 0).sum() < speed.sum()   # oracle: 60 and 135 of 540
    lattice = s["family"] == gen.BALL_LATTICE
    assert (run["B"][lattice, 0, 1] > 0).sum() >= 35   # oracle: 72 rows bail on dist == 0 at the first tick


def test_census_ball_pair(run):
    """first-creation repulsion (entity_death_ball.py:153-166): groups in which the pair's distance 16 is straddled -- one ball's
    speed jumps by 4 px per tick"""
    s = gen.states()
    rows = np.nonzero(s["family"] == gen.BALL_PAIR)[0]
    pushed = (np.abs(run["M"][rows, 0, :2, 2:4]).max(axis=(1, 2)) > 1).reshape(-1, 5)
    both = int((pushed.any(axis=1) & ~pushed.all(axis=1)).sum())
    print("ball_pair groups %d: repelled in some rows and not in others in %d; repelled in all rows of %d" % (len(pushed), both, int(pushed.all(axis=1).sum())))
    assert both >= 7 and pushed.all(axis=1).sum() >= 16   # oracle: 14 and 32


def test_census_thwump_and_drone(run):
    """thwump rows: crushed and surviving at neighbouring gaps; retreating thwumps that stop on their origin and that pass it;
    charging thwumps stopped by the border and not; drones that take a new direction at the first tick and that fly on"""
    s = gen.states()
    rows = np.nonzero(s["family"] == gen.THWUMP)[0]
    dead = np.isin(run["D"][rows][:, :, 0], (6, 7)).any(axis=1)
    crush = (s["xyv"][rows, 1] == 254.0) & (s["mfield"][rows, 0] == -1)
    # one series of gaps per (thwump, ninja x): against the floor at two ninja positions, against the wall; inside a series the rows
    # are in the order of their gaps
    series = np.stack([s["mslot"][rows, 0], s["xyv"][rows, 0]], axis=1)[crush]
    keys = np.unique(series, axis=0)
    assert len(keys) == 3
    flips = []
    for k in keys:
        d = dead[crush][(series == k).all(axis=1)]
        flips.append(int((np.diff(d.astype(int)) != 0).sum()))
        print("crush series (slot %d, ninja x %.1f): %d rows, dead %d, alive %d, changes between neighbouring gaps %d" % (k[0], k[1], len(d), int(d.sum()),
                                                                                                              int((~d).sum()), flips[-1]))
        assert len(d) == 41 and d.sum() >= 15 and (~d).sum() >= 4 and flips[-1] >= 1   # oracle: dead 33, 30, 31; alive 8, 11, 10
    assert sum(flips) >= 4   # oracle: 3 + 3 + 1
    slot = s["mslot"][rows, 0]
    state0 = run["M"][rows, 0, slot, 4]   # the set thwump's state after the first tick
    back = (s["mfield"][rows, 0] == -1) & ~crush
    fwd = s["mfield"][rows, 0] == 1
    print("retreating: stopped (state 0) %d, still retreating %d; charging: still charging %d, turned back %d"
          % (int((state0[back] == 0).sum()), int((state0[back] == -1).sum()), int((state0[fwd] == 1).sum()), int((state0[fwd] == -1).sum())))
    assert (state0[back] == 0).sum() >= 8 and (state0[back] == -1).sum() >= 40     # oracle: 16 and 84
    assert (state0[fwd] == 1).sum() >= 28 and (state0[fwd] == -1).sum() >= 8       # oracle: 57 and 16
    rows = np.nonzero(s["family"] == gen.DRONE)[0]
    slot = s["mslot"][rows, 0]
    arrived = (run["M"][rows, 0, slot, 2] != s["mxyab"][rows, 0, 2]) | (run["M"][rows, 0, slot, 3] != s["mxyab"][rows, 0, 3])   # a new target
    print("drone rows %d: new target at the first tick %d, flying on %d" % (len(rows), int(arrived.sum()), int((~arrived).sum())))
    assert arrived.sum() >= 35 and (~arrived).sum() >= 16   # oracle: 72 and 32


def test_mover_aids_on_the_host(oracle_mod):
    """the two aids' ABI (header, export list, null handle) and the oracle's side of them: Oracle.set_mover writes the four doubles and
    the field of one mover -- not Entity.cell, not another mover, not the ninja -- and a refusal writes nothing"""
    import ctypes as C
    import os
    import re

    from nclone_amd import _native as native

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "npp_amd.h")).read()
    assert re.search(r"int npp_set_mover_state\(npp_handle h, int env0, int count, int slot, const double \*xyab", hdr)
    assert re.search(r"int npp_dump_movers\(npp_handle h, int env, double \*out", hdr)
    assert "TEST AID" in hdr[hdr.index("int npp_set_mover_state") - 1400:hdr.index("int npp_set_mover_state")]
    lib = native.lib()
    assert {"npp_set_mover_state", "npp_dump_movers"} <= set(native.EXPORTS)
    xyab = (C.c_double * 4)(1.0, 2.0, 0.0, 0.0)
    assert lib.npp_set_mover_state(None, 0, 1, 0, xyab, None) == native.NPP_ERR_INVALID
    assert lib.npp_dump_movers(None, 0, xyab, 0, None) == native.NPP_ERR_INVALID
    o = oracle_mod.Oracle("pow")
    o.load(gen.level_maps()[gen.MOVERS])
    o.reset()
    slot = {t: k for k, t, _, _, _ in gen.movers(gen.MOVERS)}
    m0, e0, c0 = o.dump_movers(), o.dump_entities(), o.core()
    o.set_mover(slot[20], 333.25, 111.5, 0.0, 0.0, -1)
    o.set_mover(slot[14], 400.0, 210.0, 424.0, 210.0, 3)
    o.set_mover(slot[25], 700.0, 99.0, -3.25, -0.0)
    want = m0.copy()
    want[slot[20]] = [333.25, 111.5, 0.0, 0.0, -1]
    want[slot[14]] = [400.0, 210.0, 424.0, 210.0, 3]
    want[slot[25], :4] = [700.0, 99.0, -3.25, -0.0]
    m1, e1 = o.dump_movers(), o.dump_entities()
    assert np.array_equal(m1.view(np.int64), want.view(np.int64))
    assert np.array_equal(e1[:, 4:], e0[:, 4:]) and np.array_equal(e1[:, :2], e0[:, :2])   # cells, states, active: as before
    assert np.array_equal(o.core()[0], c0[0]) and np.array_equal(o.core()[1], c0[1])
    for args in ((len(slot) + 3, 1.0, 2.0, 0.0, 0.0), (-1, 1.0, 2.0, 0.0, 0.0), (slot[20], 1.0, 2.0, 0.0, 0.0, 2), (slot[14], 1.0, 2.0, 3.0, 4.0, 4),
                 (slot[25], 1.0, 2.0, 3.0, 4.0, 0), (slot[28], 1.0, 2.0, 0.0, 0.0, 1), (slot[20], 1.0, 2.0, 3.0, 0.0), (slot[17], np.nan, 2.0, 0.0, 0.0),
                 (slot[17], 1.0, 2.0, np.inf, 0.0)):
        with pytest.raises(ValueError):
            o.set_mover(*args)
        assert np.array_equal(o.dump_movers().view(np.int64), m1.view(np.int64))
