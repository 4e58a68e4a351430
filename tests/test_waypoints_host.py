"""CPU checks of the sequential path waypoints of reward mode "pbrs" (include/npp_amd.h npp_set_reward_waypoints): the
per-level table (npp_reward_waypoints_host: the two optimal paths and the waypoints along them) and the rule the device kernel runs
(npp_waypoint.hpp, through npp_reward_host_wp) against tests/golden/waypoints.npz -- paths, waypoints, rewards, bonuses and collection
state produced by running the reference's RewardCalculator under a fresh RewardConfig().  The expectation is EXACT equality of the
tables and BIT equality of every fp64 number."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
END_BITS = 3   # the fixture's episodes end on win / death (no truncation occurs in them)


@pytest.fixture(scope="module")
def lib():
    from nclone_amd import build_native

    build_native.build()
    from nclone_amd import _native

    return _native.lib()


@pytest.fixture(scope="module")
def fix():
    z = np.load(os.path.join(ROOT, "tests", "golden", "waypoints.npz"))
    return z, bytes(z["names"]).decode().split("\n")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_table(lib, m, spacing=12.0, cap=600):
    """-> (rc, status, table f64[count, 4] as the fixture's wp<k>, path0, path1, nodes)"""
    m = np.ascontiguousarray(m, dtype=np.float64)
    xy, ph, ni = np.full((cap, 2), np.nan), np.full(cap, 255, dtype=np.uint8), np.full(cap, -1, dtype=np.int32)
    p0, p1 = np.full((2000, 2), -1, dtype=np.int32), np.full((2000, 2), -1, dtype=np.int32)
    plen, nodes = np.full(2, -1, dtype=np.int32), np.full((3, 2), -7, dtype=np.int32)
    st = np.full(1, -1, dtype=np.int32)
    count = C.c_int32(-1)
    rc = lib.npp_reward_waypoints_host(m.ctypes.data_as(C.POINTER(C.c_double)), m.size, spacing, cap, _p(xy), _p(ph), _p(ni), C.byref(count),
                                       2000, _p(p0), _p(p1), _p(plen), _p(nodes), _p(st))
    n = max(count.value, 0)
    tab = np.column_stack([xy[:n], ph[:n].astype(np.float64), ni[:n].astype(np.float64)]) if rc == 0 else None
    return rc, int(st[0]), tab, p0[:max(plen[0], 0)], p1[:max(plen[1], 0)], nodes


def host_reward_wp(lib, m, pos, flags, frames, wp=None, params=None, end_bits=END_BITS):
    """pos [steps + 1, 2]: row 0 the reset observation; wp: None = waypoints off, else the four numbers
    -> (rc, reward, components, kind, bonus f64[steps], info i32[steps, 3])"""
    m = np.ascontiguousarray(m, dtype=np.float64)
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    flags = np.ascontiguousarray(flags, dtype=np.uint8)
    frames = np.ascontiguousarray(frames, dtype=np.uint16)
    n = len(flags)
    assert pos.shape == (n + 1, 2) and len(frames) == n
    rew, comp, kind = np.full(n, np.nan), np.full((n, 6), np.nan), np.full(n, 255, dtype=np.uint8)
    bonus, info = np.full(n, np.nan), np.full((n, 3), -9, dtype=np.int32)
    st = np.full(1, -1, dtype=np.int32)
    par = None if params is None else np.ascontiguousarray(params, dtype=np.float64)
    w = None if wp is None else np.ascontiguousarray(wp, dtype=np.float64)
    rc = lib.npp_reward_host_wp(m.ctypes.data_as(C.POINTER(C.c_double)), m.size, _p(par), _p(w), _p(pos[:1].copy()), _p(np.ascontiguousarray(pos[1:])),
                                _p(flags), _p(frames), n, end_bits, _p(rew), _p(comp), _p(kind), _p(st), _p(bonus), _p(info))
    return rc, rew, comp, kind, bonus, info


def rollouts(z, k):
    """(prefix, pos, flags, frames, waypoint numbers) of level k's rollouts; rollout "c" shares rollout "a"'s trajectory"""
    for pre in "abce":
        if "%srew%d" % (pre, k) in z.files:
            src = "a" if pre == "c" else pre
            yield pre, z["%spos%d" % (src, k)], z["%sflags%d" % (src, k)], z["%sframes%d" % (src, k)], (z["params_wp_c"] if pre == "c" else z["params_wp"])


def accepted(z, names):
    return [k for k in range(len(names)) if not np.isinf(z["const%d" % k]).any()]


def test_fixture_covers_the_cases(fix):
    z, names = fix
    assert len(names) == 7 and len(accepted(z, names)) == 6
    assert z["farm_distance_none"].tolist() == [1]   # the farming penalty's distance is never in the observation: always 0
    cover = dict(in_sequence=0, out_skip=0, out_backwards=0, death_collected=0, restart_after_collection=0, scripted=0, nondefault=0)
    for k in accepted(z, names):
        for pre, _pos, flags, _fr, _wp in rollouts(z, k):
            info = z["%swpi%d" % (pre, k)]
            assert not z["%sfarm%d" % (pre, k)].any()
            nxt0 = np.concatenate([[0], np.where((flags[:-1] & 3) != 0, 0, info[:-1, 2])])   # next expected before the step
            cover["in_sequence"] += int((info[:, 1] == 1).sum())
            cover["out_skip"] += int(((info[:, 1] == 2) & (info[:, 0] > nxt0)).sum())
            cover["out_backwards"] += int(((info[:, 1] == 2) & (info[:, 0] + 1 < nxt0)).sum())
            cover["death_collected"] += int((((flags & 2) != 0) & (info[:, 3] > 0)).sum())
            cover["restart_after_collection"] += int((((flags & 3) != 0) & (info[:, 3] > 0))[:-1].sum())
            cover["scripted"] += pre == "e"
            cover["nondefault"] += pre == "c"
    assert all(v >= 1 for v in cover.values()), cover


def test_default_params_are_the_recorded_ones(lib, fix):
    z, _ = fix
    q = (C.c_double * 4)()
    lib.npp_waypoint_default_params(q)
    assert list(q) == z["params_wp"].tolist() == [18.0, 0.3, 2.0, 12.0]


def test_tables_and_paths_equal_the_reference(lib, fix):
    z, names = fix
    refused = 0
    for k, tag in enumerate(names):
        rc, st, tab, p0, p1, nodes = host_table(lib, z["m%d" % k])
        if np.isinf(z["const%d" % k]).any():   # the reference raises on this level: the mode refuses it, and so do the waypoints
            assert rc == 3 and st == 2 and tag == "mines:replay:91", (tag, rc, st)
            refused += 1
            continue
        assert rc == 0 and st == 0, (tag, rc, st)
        assert np.array_equal(nodes, z["nodes%d" % k]), (tag, nodes.tolist(), z["nodes%d" % k].tolist())
        assert np.array_equal(p0, z["path0_%d" % k]), (tag, "spawn -> switch")
        assert np.array_equal(p1, z["path1_%d" % k]), (tag, "switch -> exit")
        want = z["wp%d" % k]
        assert tab.shape == want.shape and np.array_equal(tab, want), (tag, tab.tolist(), want.tolist())
    assert refused == 1


def test_every_fixture_row_bit_for_bit(lib, fix):
    z, names = fix
    rows = collected = 0
    for k in accepted(z, names):
        tag = names[k]
        for pre, pos, flags, frames, wp in rollouts(z, k):
            rc, rew, comp, kind, bonus, info = host_reward_wp(lib, z["m%d" % k], pos, flags, frames, wp)
            assert rc == 0, (tag, pre)
            want = z["%srew%d" % (pre, k)]
            bad = np.flatnonzero(rew.view(np.uint64) != want.view(np.uint64))
            assert len(bad) == 0, (tag, pre, len(bad), bad[:5], rew[bad[:5]], want[bad[:5]])
            assert np.array_equal(kind, z["%skind%d" % (pre, k)]), (tag, pre)
            ref = z["%scomp%d" % (pre, k)]
            live = kind != 3
            assert np.array_equal(comp[:, 0], ref[:, 0]) and np.array_equal(comp[:, 3], ref[:, 2]), (tag, pre)
            assert np.array_equal(np.where(live, comp[:, 1], comp[:, 2]), ref[:, 1]), (tag, pre)
            assert np.array_equal(comp[:, 4], ref[:, 3]), (tag, pre)
            wb, wi = z["%swpb%d" % (pre, k)], z["%swpi%d" % (pre, k)]
            assert np.array_equal(bonus.view(np.uint64), wb.view(np.uint64)), (tag, pre, np.flatnonzero(bonus != wb)[:5])
            assert np.array_equal(info, wi[:, [0, 2, 3]]), (tag, pre, np.flatnonzero((info != wi[:, [0, 2, 3]]).any(axis=1))[:5])
            rows += len(want)
            collected += int((wi[:, 0] >= 0).sum())
    assert rows > 2700 and collected > 150


def test_bonus_formula_equals_the_recorded_grid(lib, fix):
    z, _ = fix
    out = C.c_double()
    got = []
    for i, total, inseq, scale, oscale in z["grid_in"]:
        assert lib.npp_waypoint_bonus_host(int(i), int(total), int(inseq), scale, oscale, C.byref(out)) == 0
        got.append(out.value)
    got = np.array(got)
    assert {1, 20, 21, 62} <= set(z["grid_in"][:, 1].astype(int).tolist())
    assert np.array_equal(got.view(np.uint64), z["grid_out"].view(np.uint64)), np.flatnonzero(got != z["grid_out"])[:5]


def test_waypoints_off_is_npp_reward_host(lib):
    from tests.test_reward_host import host_reward
    from tests.test_reward_host import rollouts as reward_rollouts

    z = np.load(os.path.join(ROOT, "tests", "golden", "reward.npz"))
    rows = 0
    for k in range(7):
        if np.isinf(z["const%d" % k]).any():
            continue
        for pre, pos, flags, frames, par in reward_rollouts(z, k):
            rc0, rew0, comp0, kind0 = host_reward(lib, z["m%d" % k], pos, flags, frames, par)
            rc, rew, comp, kind, bonus, info = host_reward_wp(lib, z["m%d" % k], pos, flags, frames, None, par)
            assert rc0 == rc == 0
            assert np.array_equal(rew.view(np.uint64), rew0.view(np.uint64)) and np.array_equal(rew.view(np.uint64), z["%srew%d" % (pre, k)].view(np.uint64))
            assert np.array_equal(comp, comp0) and np.array_equal(kind, kind0)
            assert np.isnan(bonus).all() and (info == -9).all()   # not written
            rows += len(rew)
    assert rows > 2800


def test_refusals(lib, fix):
    z, names = fix
    k = names.index("mines:replay:24")
    pos, flags, frames = z["apos%d" % k][:9], z["aflags%d" % k][:8], z["aframes%d" % k][:8]
    assert host_reward_wp(lib, z["m%d" % k], pos, flags, frames, [24.0, 0.3, 2.0, 12.0])[0] == 0
    assert host_reward_wp(lib, z["m%d" % k], pos, flags, frames, [24.5, 0.3, 2.0, 12.0])[0] == 1   # NPP_ERR_INVALID: beyond the cell walk
    assert host_reward_wp(lib, z["m%d" % k], pos, flags, frames, [-1.0, 0.3, 2.0, 12.0])[0] == 1
    assert host_reward_wp(lib, z["m%d" % k], pos, flags, frames, [18.0, np.nan, 2.0, 12.0])[0] == 1
    assert host_reward_wp(lib, z["m%d" % k], pos, flags, frames, [18.0, 0.3, 2.0, 0.0])[0] == 1
    assert host_table(lib, z["m%d" % k][:100])[0] == 1
    # a wider spacing thins the table; the level with a single waypoint keeps none at 40 px
    rc, _st, tab, _p0, _p1, _n = host_table(lib, z["m%d" % k], spacing=30.0)
    assert rc == 0 and 0 < len(tab) < len(z["wp%d" % k])
    k0 = names.index("c0:replay:0")
    rc, _st, tab, p0, _p1, _n = host_table(lib, z["m%d" % k0], spacing=40.0)
    assert rc == 0 and len(tab) == 0 and len(p0) == len(z["path0_%d" % k0])
    rc, rew, _c, _k, bonus, info = host_reward_wp(lib, z["m%d" % k0], z["apos%d" % k0], z["aflags%d" % k0], z["aframes%d" % k0], [18.0, 0.3, 2.0, 40.0])
    assert rc == 0 and not bonus.any() and (info[:, 0] == -1).all()   # a level without waypoints: the bonus is always 0


def test_host_entries_under_asan_and_ubsan(fix, tmp_path):
    """npp_reward_waypoints_host and npp_reward_host_wp in a stand-alone program (tests/waypoints_sanitized_main.cpp) built with
    g++ -fsanitize=address,undefined together with the host sources, runtimes linked statically: on three fixture levels it must print
    the fixture's table sizes and rewards, on every 37th prefix of each map and on a map whose entity counts lie it must not fault,
    and no sanitizer report may appear."""
    import subprocess

    from nclone_amd import build_native

    z, names = fix
    exe = str(tmp_path / "waypoints_sanitized_main")
    srcs = [os.path.join(build_native.CSRC, f) for f in build_native.HOST_SOURCES]
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-static-libasan",
                        "-static-libubsan", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "waypoints_sanitized_main.cpp")] + srcs + ["-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=23", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for tag, pre in (("c0:replay:20", "a"), ("mines:replay:24", "e"), ("zoo:replay:16", "b")):
        k = names.index(tag)
        pos, flags, frames = z["%spos%d" % (pre, k)], z["%sflags%d" % (pre, k)], z["%sframes%d" % (pre, k)]
        files = {}
        for name, a, dt in (("map", z["m%d" % k], np.float64), ("pos", pos, np.float64), ("flags", flags, np.uint8), ("frames", frames, np.uint16)):
            files[name] = str(tmp_path / (name + ".bin"))
            np.ascontiguousarray(a, dtype=dt).tofile(files[name])
        r = subprocess.run([exe, files["map"], files["pos"], files["flags"], files["frames"], str(len(flags)), str(END_BITS)],
                           capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, (tag, r.returncode, r.stdout[-500:], r.stderr[-3000:])
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
        out = r.stdout.split("\n")
        want = z["wp%d" % k]
        assert out[0].split() == ["table", "0", "0", str(len(want)), str(int((want[:, 2] == 0).sum())), str(len(z["path0_%d" % k])),
                                  str(len(z["path1_%d" % k]))], (tag, out[0])
        assert out[1] == "rewards 0"
        rows = [l.split() for l in out[2:2 + len(flags)]]
        rew = np.array([float.fromhex(a) for a, _b, _c in rows])
        assert np.array_equal(rew.view(np.uint64), z["%srew%d" % (pre, k)].view(np.uint64)), tag
        bonus = np.array([float.fromhex(b) for _a, b, _c in rows])
        assert np.array_equal(bonus.view(np.uint64), z["%swpb%d" % (pre, k)].view(np.uint64)), tag
        assert np.array_equal(np.array([int(c) for _a, _b, c in rows]), z["%swpi%d" % (pre, k)][:, 0]), tag
        assert int(out[-2].split()[-1]) >= 30, out[-2]   # the malformed maps were refused


def test_header_declares_the_entry_points():
    h = open(os.path.join(ROOT, "include", "npp_amd.h")).read()
    for name in ("npp_set_reward_waypoints", "npp_set_waypoint_params", "npp_step_reward_wp", "npp_reward_waypoints", "npp_waypoint_default_params",
                 "npp_reward_waypoints_host", "npp_reward_host_wp", "npp_waypoint_bonus_host"):
        assert re.search(r"\b%s\(" % name, h), name
    assert "typedef struct NppWaypointParams" in h
