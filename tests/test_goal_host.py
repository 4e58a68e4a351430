"""CPU checks of the goal curriculum (include/npp_amd.h npp_set_goal_curriculum): the stage table
(npp_goal_stages_host) against tests/golden/goal.npz -- paths, distances, stage counts and positions produced by running the
reference's IntermediateGoalManager -- with BIT equality of every fp64 number; the variant compile against the cells the reference's
apply_to_simulator left; and the bookkeeping rule (npp_goal_apply_host) against the plain Python restatement tests/goal_ref.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import goal_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EK_EXIT, EK_SWITCH = 3, 4


@pytest.fixture(scope="module")
def lib():
    from nclone_amd import build_native

    build_native.build()
    from nclone_amd import _native

    return _native.lib()


@pytest.fixture(scope="module")
def fix():
    z = np.load(os.path.join(ROOT, "tests", "golden", "goal.npz"))
    return z, bytes(z["names"]).decode().split("\n")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _map(m):
    m = np.ascontiguousarray(m, dtype=np.float64)
    return m, m.ctypes.data_as(C.POINTER(C.c_double))


def stages(lib, m, interval, cap=64):
    m, mp = _map(m)
    ns, dist, orig, pos = np.full(1, -9, dtype=np.int32), np.full(3, np.nan), np.full(4, np.nan), np.full((cap, 4), np.nan)
    p0, p1, plen = np.full((2000, 2), -1, dtype=np.int32), np.full((2000, 2), -1, dtype=np.int32), np.full(2, -1, dtype=np.int32)
    rc = lib.npp_goal_stages_host(mp, m.size, float(interval), _p(ns), _p(dist), _p(orig), cap, _p(pos), 2000, _p(p0), _p(p1), _p(plen))
    return rc, int(ns[0]), dist, orig, pos[:max(int(ns[0]), 1)], p0[:max(plen[0], 0)], p1[:max(plen[1], 0)]


def entities(lib, m, goal_xy=None):
    m, mp = _map(m)
    out, order, n = np.zeros((4096, 6)), np.full((4096, 4), -1, dtype=np.int32), C.c_int(-1)
    g = None if goal_xy is None else np.ascontiguousarray(goal_xy, dtype=np.float64)
    assert lib.npp_compile_level_entities_goal(mp, m.size, _p(g), _p(out), 4096, C.byref(n), _p(order)) == 0
    return out[:n.value], order[:n.value]


def segments(lib, m, goal_xy=None):
    m, mp = _map(m)
    out, n = np.zeros((20000, 8), dtype=np.int16), C.c_int(-1)
    g = None if goal_xy is None else np.ascontiguousarray(goal_xy, dtype=np.float64)
    assert lib.npp_compile_level_segments_goal(mp, m.size, _p(g), _p(out), 20000, C.byref(n), None) == 0
    return out[:n.value]


def test_fixture_covers_the_cases(fix):
    z, names = fix
    assert len(names) == 7 and z["interval"].tolist() == [100.0, 48.0]
    # the stage counts the issue measured at interval 100
    assert [int(z["astages%d" % k][0]) for k in range(7)] == [2, 2, 0, 7, 2, 2, 5]
    assert max(int(z["bstages%d" % k][0]) for k in range(7)) == 14 and int(z["bstages0"][0]) == 3
    # quirk 1: the last stage is the paths' end nodes, not the map positions
    assert z["apos0"][-1].tolist() == [834.0, 486.0, 822.0, 486.0] and z["orig0"].ravel().tolist() == [834.0, 492.0, 828.0, 492.0]
    # quirk 3: a one-node second path puts both entities on one spot at every stage
    assert len(z["path1_1"]) == 1 and all(r[:2].tolist() == r[2:].tolist() for r in z["apos1"])
    cells = np.stack([z["rcell%d" % r] for r in range(len(z["roll_level"]))])
    assert (cells[:, 0, 0] != cells[:, 0, 1]).any() and (cells[:, 0, 0] == cells[:, 0, 1]).any() and (cells[:, 1, 0] != cells[:, 1, 1]).any()
    assert any((z["rd%d" % r][:, 0] == 8).any() for r in range(len(z["roll_level"])))
    assert z["same_tick_wins"].tolist() == [0]


def test_stage_table_is_the_references_bit_for_bit(lib, fix):
    z, names = fix
    for k, tag in enumerate(names):   # all seven, none skipped: mines:replay:91 is the level without stages
        for q, interval in zip("ab", z["interval"]):
            rc, ns, dist, orig, pos, p0, p1 = stages(lib, z["m%d" % k], interval)
            assert rc == 0, (tag, q)
            assert ns == int(z["%sstages%d" % (q, k)][0]), (tag, q, ns)
            assert np.array_equal(p0, z["path0_%d" % k]) and np.array_equal(p1, z["path1_%d" % k]), (tag, q)
            assert np.array_equal(dist.view(np.uint64), z["%sdist%d" % (q, k)].view(np.uint64)), (tag, q, dist)
            assert np.array_equal(orig.reshape(2, 2), z["orig%d" % k]), (tag, q)
            assert np.array_equal(pos.view(np.uint64), z["%spos%d" % (q, k)].view(np.uint64)), (tag, q, pos)
    k = names.index("mines:replay:91")
    assert stages(lib, z["m%d" % k], 100.0)[1] == 0 and len(z["path0_%d" % k]) > 0 and len(z["path1_%d" % k]) == 0
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert stages(lib, z["m0"], bad)[0] != 0
    assert stages(lib, z["m3"], 0.5)[0] != 0   # more than 1024 stages


def test_variant_compile_carries_apply_to_simulator(lib, fix):
    z, names = fix
    for k in range(7):
        m = z["m%d" % k]
        base_seg, (base_ent, base_ord) = segments(lib, m), entities(lib, m)
        e0, o0 = entities(lib, m, None)
        assert np.array_equal(e0, base_ent) and np.array_equal(o0, base_ord)
        for row in z["apos%d" % k][: max(int(z["astages%d" % k][0]), 0)]:
            assert np.array_equal(segments(lib, m, row), base_seg)   # tiles, hence segments, are the base level's
            ent, order = entities(lib, m, row)
            assert len(ent) == len(base_ent)
            sw, door = int(np.flatnonzero(ent[:, 0] == EK_SWITCH)[-1]), int(np.flatnonzero(ent[:, 0] == EK_EXIT)[-1])
            assert ent[sw, 1:3].tolist() == row[:2].tolist() and ent[door, 1:3].tolist() == row[2:].tolist()
            for i, (x, y) in ((sw, row[:2]), (door, row[2:])):   # clamp_cell(floor(x / 24), floor(y / 24))
                assert ent[i, 3:5].tolist() == [min(max(np.floor(x / 24), 0), 43), min(max(np.floor(y / 24), 0), 24)]
            others = [i for i in range(len(ent)) if i not in (sw, door)]
            assert np.array_equal(ent[others], base_ent[others])   # nothing else moved
            moved = ent[sw, 3:5].tolist() != base_ent[sw, 3:5].tolist()
            same_cell = [i for i in range(len(ent)) if ent[i, 3:5].tolist() == ent[sw, 3:5].tolist() and ent[i, 0] != EK_EXIT and i != sw]
            if moved:   # appended: behind every load-time entity of the new cell, in both reset orders, with the first free number
                assert all(order[i, 0] < order[sw, 0] and order[i, 1] < order[sw, 1] and order[i, 2] < order[sw, 2] and order[i, 3] < order[sw, 3]
                           for i in same_cell)
                assert order[sw, 1] == order[sw, 2] == len(ent) + _n_movers(lib, m)
            else:       # stays where it was in its list
                assert np.array_equal(order[sw, 1:3], base_ord[sw, 1:3])
            in_door_cell = [i for i in range(len(ent)) if ent[i, 3:5].tolist() == ent[door, 3:5].tolist() and ent[i, 0] != EK_EXIT]
            assert all(order[i, 0] < order[door, 0] and order[i, 3] < order[door, 3] for i in in_door_cell)   # "exit doors last"
    # the cells the reference's own apply_to_simulator left on a live simulator
    for r in range(len(z["roll_level"])):
        k, s = int(z["roll_level"][r]), int(z["roll_stage"][r])
        ent, _ = entities(lib, z["m%d" % k], z["apos%d" % k][s])
        base_ent, _ = entities(lib, z["m%d" % k])
        sw, door = int(np.flatnonzero(ent[:, 0] == EK_SWITCH)[-1]), int(np.flatnonzero(ent[:, 0] == EK_EXIT)[-1])
        got = [[base_ent[i, 3] * 25 + base_ent[i, 4], ent[i, 3] * 25 + ent[i, 4]] for i in (sw, door)]
        assert got == z["rcell%d" % r].tolist(), (r, got)


def _n_movers(lib, m):
    m, mp = _map(m)
    edges, n = np.zeros(2 * 89 * 51, dtype=np.int32), C.c_int(-1)
    assert lib.npp_compile_level_zoo(mp, m.size, edges.ctypes.data_as(C.POINTER(C.c_int32)), None, 0, C.byref(n)) == 0
    return n.value


def _apply_host(lib, ref_like, lv, ring, env, flags, level, drawn, count, auto=1):
    changed = np.full(len(flags), 7, dtype=np.uint8)
    d = None if drawn is None else np.ascontiguousarray(drawn, dtype=np.int32)
    rc = lib.npp_goal_apply_host(_p(lv), _p(ring), _p(env), _p(ref_like.base_of), _p(ref_like.stage_of), ref_like.nb, len(ref_like.base_of),
                                 ref_like.n, ref_like.window, ref_like.need, auto, _p(flags), gr.END_BITS, 1 if count else 0, _p(level), _p(d), _p(changed))
    assert rc == 0
    return changed


def test_rule_equals_the_python_restatement(lib):
    """Generated event streams: several ends of one level in one step, stale-stage episodes, a pending stage, a ring wrap, an advance at
    exactly `need` wins and none at need - 1, the last stage, explicit restarts (count = 0) and pool draws."""
    rng = np.random.default_rng(25)
    num_stages, n, window = [3, 0, 2, 5], 23, 4
    need = gr.need_for(window, 0.5)
    assert need == 2 and gr.need_for(500, 0.80) == 400 and gr.need_for(3, 0.5) == 2 and gr.need_for(4, 1.0) == 4 and gr.need_for(7, 0.0) == 0
    ref = gr.GoalRef(num_stages, n, window, need)
    lv, ring, env = ref.lv.copy(), ref.ring.copy(), ref.env.copy()
    level = np.array([ref.level_for(b) for b in rng.integers(0, 4, size=n)], dtype=np.int32)
    level_h = level.copy()
    for step in range(400):
        flags = rng.choice(np.array([0, 0, 0, 4, 4, 1 | 4, 2, 2 | 4, 8, 1], dtype=np.uint8), size=n)
        if step < 40:
            flags[flags == 5] = 2   # no wins at first: rings fill and wrap without advancing
        drawn = rng.integers(0, 4, size=n).astype(np.int32) if step % 3 == 0 else None
        count = step % 11 != 5
        if step in (60, 200):
            ref.set_stage(9 if step == 60 else 0, None if step == 60 else 3)
            lv[gr.PENDING] = ref.lv[gr.PENDING]
        want_changed = ref.apply(flags, level, drawn, count)
        got_changed = _apply_host(lib, ref, lv, ring, env, flags, level_h, drawn, count)
        assert np.array_equal(lv, ref.lv) and np.array_equal(ring, ref.ring) and np.array_equal(env, ref.env), step
        assert np.array_equal(level_h, level) and np.array_equal(got_changed, want_changed), step
        assert (lv[gr.STAGE] <= np.maximum(np.array(num_stages) - 1, 0)).all() and lv[gr.STAGE, 1] == 0 and lv[gr.FILL, 1] == 0
    ev = ref.events
    assert ev["advance"] >= 1 and ev["wrap"] >= 1 and ev["stale"] >= 1 and ev["pending"] >= 1 and ev["pinned"] >= 1, ev
    assert (ref.env[gr.SWITCHES] >= ref.env[gr.COMPLETIONS]).all() and (ref.env[gr.EPISODES] >= ref.env[gr.SWITCHES]).all()


def test_advance_at_exactly_need_and_not_below(lib):
    window, need = 4, 3
    for wins, advanced in ((need - 1, False), (need, True)):
        ref = gr.GoalRef([3], window, window, need)
        lv, ring, env = ref.lv.copy(), ref.ring.copy(), ref.env.copy()
        level = np.full(window, ref.level_for(0), dtype=np.int32)
        flags = np.array([1] * wins + [2] * (window - wins), dtype=np.uint8)   # all of one level end in one step, in env order
        ref.apply(flags, level.copy())
        _apply_host(lib, ref, lv, ring, env, flags, level, None, True)
        assert np.array_equal(lv, ref.lv) and int(lv[gr.STAGE, 0]) == int(advanced) and int(lv[gr.FILL, 0]) == (0 if advanced else window)
        assert level.tolist() == [ref.lv[gr.VARIANT0, 0] + int(advanced)] * window
    # auto_advance off: a full ring of wins never advances
    ref = gr.GoalRef([3], window, window, need, auto_advance=False)
    lv, ring, env = ref.lv.copy(), ref.ring.copy(), ref.env.copy()
    level = np.full(window, ref.level_for(0), dtype=np.int32)
    flags = np.full(window, 1, dtype=np.uint8)
    ref.apply(flags, level.copy())
    _apply_host(lib, ref, lv, ring, env, flags, level, None, True, auto=0)
    assert np.array_equal(lv, ref.lv) and lv[gr.STAGE, 0] == 0 and lv[gr.WINS, 0] == window


def test_explicit_restart_drops_the_switch_latch(lib):
    """an env hits the switch, is restarted explicitly (count = 0), then dies without the switch: no activation is counted"""
    ref = gr.GoalRef([3], 1, 4, 2)
    lv, ring, env = ref.lv.copy(), ref.ring.copy(), ref.env.copy()
    level = np.array([ref.level_for(0)], dtype=np.int32)
    for flags, count in (([4], True), ([1], False), ([2], True)):   # (the restart's "flags" are its mask: any end bit)
        f = np.array(flags, dtype=np.uint8)
        ref.apply(f, level.copy(), None, count)
        _apply_host(lib, ref, lv, ring, env, f, level, None, count)
        assert np.array_equal(env, ref.env) and np.array_equal(lv, ref.lv)
    assert env[gr.EPISODES, 0] == 1 and env[gr.SWITCHES, 0] == 0 and env[gr.SEEN, 0] == 0


def _variant(z, r):
    k, st = int(z["roll_level"][r]), int(z["roll_stage"][r])
    m, mp = _map(z["m%d" % k])
    return m, mp, np.ascontiguousarray(z["apos%d" % k][st], dtype=np.float64)


def test_reach_features_and_path_direction_on_variants(lib, fix):
    """the host twins with the override argument against the rows the reference computed on the moved LevelData, the manager handed
    to its path calculator: every recomputed feature row bit for bit, every direction and from-graph bit"""
    z, _names = fix
    rows = 0
    for r in range(len(z["roll_level"])):
        m, mp, g = _variant(z, r)
        pos, mines = np.ascontiguousarray(z["op%d" % r]), np.ascontiguousarray(z["od%d" % r], dtype=np.int32)
        new_ep = np.zeros(len(pos), dtype=np.uint8)
        new_ep[1:] = z["ot%d" % r]
        out, st = np.full((len(pos), 38), np.nan, dtype=np.float32), np.full(len(pos), -1, dtype=np.int32)
        assert lib.npp_reach_rollout_goal_host(mp, m.size, _p(g), _p(pos), _p(mines), _p(new_ep), len(pos), _p(out), _p(st), None) == 0
        rec = z["oc%d" % r] == 1
        assert (st == 0).all() and rec.sum() >= 10
        assert np.array_equal(out[rec].view(np.uint32), z["of%d" % r][rec].view(np.uint32)), r
        sw = np.ascontiguousarray(z["os%d" % r])
        d, gr, s1 = np.full(len(pos), -9, dtype=np.int8), np.full(len(pos), 9, dtype=np.uint8), np.full(1, -1, dtype=np.int32)
        assert lib.npp_path_direction_goal_host(mp, m.size, _p(g), _p(pos), _p(sw), len(pos), _p(d), _p(gr), _p(s1)) == 0 and s1[0] == 0
        assert np.array_equal(d, z["odir%d" % r]) and np.array_equal(gr, z["ograph%d" % r]), r
        rows += len(pos)
        # the base level answers differently: the override is what is being tested
        assert lib.npp_reach_rollout_goal_host(mp, m.size, None, _p(pos), _p(mines), _p(new_ep), len(pos), _p(out), _p(st), None) == 0
        assert not np.array_equal(out[rec].view(np.uint32), z["of%d" % r][rec].view(np.uint32)), r
    assert rows == 804
    assert len(set(np.concatenate([z["odir%d" % r] for r in range(4)]).tolist())) >= 3


def host_reward_goal(lib, z, r, pre):
    m, mp, g = _variant(z, r)
    pos, fl, fr = (np.ascontiguousarray(z["%s%s%d" % (pre, k, r)]) for k in ("pos", "flags", "frames"))
    n = len(fl)
    rew, comp, kind, st = np.full(n, np.nan), np.full((n, 6), np.nan), np.full(n, 255, dtype=np.uint8), np.full(1, -1, dtype=np.int32)
    rc = lib.npp_reward_goal_host(mp, m.size, _p(g), None, None, _p(pos[:1].copy()), _p(np.ascontiguousarray(pos[1:])), _p(fl), _p(fr), n, 3,
                                  _p(rew), _p(comp), _p(kind), _p(st), None, None)
    return rc, rew, comp, kind, fl


def test_reward_constants_and_rewards_on_variants(lib, fix):
    """reward "pbrs" on two variants against RewardCalculator(RewardConfig(enable_path_waypoints=False), goal_curriculum_manager=mgr):
    the level constants (computed by the reference from the manager's FRACTIONAL positions, pbrs_potentials.py:952-955) and every
    reward, component and branch, bit for bit as in DESIGN.md 20"""
    z, _names = fix
    assert z["reward_params"].tolist() == [-80.0, 200.0, 100.0, 0.0, 40.0, 0.99]   # npp_reward_default_params
    rows, wins, sw_live = 0, 0, 0
    for r in z["reward_rollouts"]:
        m, mp, g = _variant(z, int(r))
        assert (g != np.round(g)).any()   # the positions a map's coord * 6 cannot carry
        c, st = np.full(3, np.nan), np.full(1, -1, dtype=np.int32)
        assert lib.npp_reward_level_constants_goal_host(mp, m.size, _p(g), _p(c), _p(st)) == 0 and st[0] == 0
        assert np.array_equal(c.view(np.uint64), z["wconst%d" % r].view(np.uint64)), (r, c)
        for pre in "wv":
            rc, rew, comp, kind, fl = host_reward_goal(lib, z, int(r), pre)
            ref, live = z["%scomp%d" % (pre, r)], (fl & 3) == 0
            assert rc == 0 and np.array_equal(rew.view(np.uint64), z["%srew%d" % (pre, r)].view(np.uint64)), (r, pre)
            assert np.array_equal(kind, z["%skind%d" % (pre, r)])
            assert np.array_equal(comp[:, 0], ref[:, 0]) and np.array_equal(comp[:, 3], ref[:, 2]) and np.array_equal(comp[:, 4], ref[:, 3])
            assert np.array_equal(np.where(live, comp[:, 1], comp[:, 2]), ref[:, 1])
            rows += len(fl)
            wins += int(((fl & 1) != 0).sum())
            sw_live += int((live[1:] & ((fl[1:] & 4) != 0) & ((fl[:-1] & 4) == 0)).sum())
    assert rows == 778 and wins >= 1 and sw_live >= 1
    # waypoints towards moved goals are not computed: the combination is refused
    m, mp, g = _variant(z, 0)
    wp = np.array([18.0, 0.3, 2.0, 12.0])
    assert lib.npp_reward_goal_host(mp, m.size, _p(g), None, _p(wp), _p(np.zeros(2)), None, None, None, 0, 3, None, None, None, None, None, None) != 0


def test_sanitized_standalone_program(fix, tmp_path):
    """The stage table, the variant compile and the rule in a stand-alone program (tests/goal_sanitized_main.cpp) built with
    g++ -fsanitize=address,undefined together with the host sources, runtimes linked statically: on three fixture levels it must print
    the fixture's table, on every 37th prefix of each map and on a map whose entity counts lie it must not fault, and no sanitizer
    report may appear."""
    import subprocess

    from nclone_amd import build_native

    z, names = fix
    exe = str(tmp_path / "goal_sanitized_main")
    srcs = [os.path.join(build_native.CSRC, f) for f in build_native.HOST_SOURCES]
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-static-libasan",
                        "-static-libubsan", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "goal_sanitized_main.cpp")] + srcs + ["-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=23", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for tag, q in (("mines:replay:24", "b"), ("zoo:replay:16", "a"), ("mines:replay:91", "a")):
        k = names.index(tag)
        path = str(tmp_path / "map.bin")
        np.ascontiguousarray(z["m%d" % k], dtype=np.float64).tofile(path)
        interval = float(z["interval"]["ab".index(q)])
        r = subprocess.run([exe, path, repr(interval)], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, (tag, r.returncode, r.stdout[-500:], r.stderr[-3000:])
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
        out = r.stdout.split("\n")
        ns = int(z["%sstages%d" % (q, k)][0])
        head = out[0].split()
        assert head[0] == "stages" and int(head[1]) == ns and [int(head[5]), int(head[6])] == [len(z["path0_%d" % k]), len(z["path1_%d" % k])]
        dist = np.array([float.fromhex(v) for v in head[2:5]])
        assert np.array_equal(dist.view(np.uint64), z["%sdist%d" % (q, k)].view(np.uint64)), tag
        rows = max(ns, 1)
        pos = np.array([[float.fromhex(v) for v in l.split()] for l in out[1:1 + rows]])
        assert np.array_equal(pos.view(np.uint64), z["%spos%d" % (q, k)].view(np.uint64)), tag
        assert out[1 + 2 * rows] == "table 0" and out[2 + 2 * rows].startswith("rule 0 ")
        assert int(out[-2].split()[-1]) >= 30, out[-2]   # the malformed maps were refused


def test_header_declares_the_entry_points():
    h = open(os.path.join(ROOT, "include", "npp_amd.h")).read()
    for name in ("npp_goal_default_params", "npp_set_goal_curriculum", "npp_goal_set_stage", "npp_goal_view", "npp_goal_tables",
                 "npp_goal_stage_positions", "npp_goal_stages_host", "npp_goal_apply_host", "npp_compile_level_segments_goal",
                 "npp_compile_level_entities_goal", "npp_reach_rollout_goal_host", "npp_path_direction_goal_host",
                 "npp_reward_level_constants_goal_host", "npp_reward_goal_host"):
        assert re.search(r"\b%s\(" % name, h), name
    assert "typedef struct NppGoalCurriculumParams" in h
