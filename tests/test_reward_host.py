"""CPU checks of reward mode "pbrs" (include/npp_amd.h npp_set_reward_mode): the rule the device kernel runs
(npp_reward.hpp, through npp_reward_host) and the per-level constants (npp_reward_level_constants_host) against
tests/golden/reward.npz -- rewards, components and position-cache branches produced by running the reference's
RewardCalculator.calculate_reward on rollouts.  The expectation is BIT equality of the fp64 reward: every operation of the rule is
a correctly rounded IEEE operation, and the one `** 2` of the reference (the approach bonus) is restated as a product, which the
grid test below compares with the reference's pow on 314 arguments."""
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
    z = np.load(os.path.join(ROOT, "tests", "golden", "reward.npz"))
    return z, bytes(z["names"]).decode().split("\n")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def level_constants(lib, m):
    m = np.ascontiguousarray(m, dtype=np.float64)
    out = np.full(3, np.nan)
    st = np.full(1, -1, dtype=np.int32)
    rc = lib.npp_reward_level_constants_host(m.ctypes.data_as(C.POINTER(C.c_double)), m.size, _p(out), _p(st))
    return rc, out, int(st[0])


def host_reward(lib, m, pos, flags, frames, params=None, end_bits=END_BITS):
    """pos [steps + 1, 2]: row 0 the reset observation; -> (rc, reward f64 [steps], components f64 [steps, 6], kind u8 [steps])"""
    m = np.ascontiguousarray(m, dtype=np.float64)
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    flags = np.ascontiguousarray(flags, dtype=np.uint8)
    frames = np.ascontiguousarray(frames, dtype=np.uint16)
    n = len(flags)
    assert pos.shape == (n + 1, 2) and len(frames) == n
    rew, comp, kind = np.full(n, np.nan), np.full((n, 6), np.nan), np.full(n, 255, dtype=np.uint8)
    st = np.full(1, -1, dtype=np.int32)
    par = None if params is None else np.ascontiguousarray(params, dtype=np.float64)
    rc = lib.npp_reward_host(m.ctypes.data_as(C.POINTER(C.c_double)), m.size, _p(par), _p(pos[:1].copy()), _p(np.ascontiguousarray(pos[1:])),
                             _p(flags), _p(frames), n, end_bits, _p(rew), _p(comp), _p(kind), _p(st))
    return rc, rew, comp, kind


def rollouts(z, k):
    """(prefix, pos, flags, frames, params) of level k's rollouts; rollout "c" shares rollout "a"'s trajectory"""
    for pre in "abcd":
        if "%srew%d" % (pre, k) in z.files:
            src = "a" if pre == "c" else pre
            yield pre, z["%spos%d" % (src, k)], z["%sflags%d" % (src, k)], z["%sframes%d" % (src, k)], (z["params_c"] if pre == "c" else None)


def test_fixture_covers_the_branches(fix):
    z, names = fix
    assert len(names) == 7 and "doors:replay:127" in names and "zoo:replay:16" in names
    kinds = np.concatenate([z[f] for f in z.files if re.fullmatch(r"[abcd]kind\d", f)])
    assert all((kinds == v).sum() >= 1 for v in (0, 1, 2, 3)), np.bincount(kinds)
    assert (kinds == 0).sum() > 500 and (kinds == 1).sum() > 1000
    cover = dict(dist_sw=0, dist_ex=0, switch_live=0, death=0, win_bonus=0, approach=0, restart=0)
    for k in range(len(names)):
        for pre, _pos, flags, _fr, par in rollouts(z, k):
            comp, kd = z["%scomp%d" % (pre, k)], z["%skind%d" % (pre, k)]
            live = kd != 3
            sw = (flags & 4) != 0
            prev_sw = np.concatenate([[False], sw[:-1] & live[:-1]])
            cover["dist_sw"] += int(((comp[:, 1] > 0) & live & ~sw).sum())
            cover["dist_ex"] += int(((comp[:, 1] > 0) & live & sw).sum())
            cover["switch_live"] += int((live & sw & ~prev_sw).sum())
            cover["death"] += int(((flags & 2) != 0).sum())
            completion = (z["params_c"] if par is not None else z["params"])[1]
            cover["win_bonus"] += int((((flags & 1) != 0) & (comp[:, 3] > completion)).sum())
            cover["approach"] += int((comp[:, 2] > 0).sum())
            cover["restart"] += int((~live[:-1]).sum())
    assert all(v >= 1 for v in cover.values()), cover


def test_default_params_are_the_recorded_ones(lib, fix):
    z, _ = fix
    q = (C.c_double * 6)()
    lib.npp_reward_default_params(q)
    assert list(q) == z["params"].tolist() == [-80.0, 200.0, 100.0, 0.0, 40.0, 0.99]
    assert z["cache_threshold_sq"].tolist() == [36.0]


def test_level_constants_equal_the_reference(lib, fix):
    z, names = fix
    refused = 0
    for k, tag in enumerate(names):
        rc, out, st = level_constants(lib, z["m%d" % k])
        want = z["const%d" % k]
        assert np.array_equal(out.view(np.uint64), want.view(np.uint64)), (tag, out.tolist(), want.tolist())
        if np.isinf(want).any():   # the reference raises "Combined geometric path distance is infinite"
            assert rc == 3 and st == 2, (tag, rc, st)
            assert host_reward(lib, z["m%d" % k], np.zeros((1, 2)), [], [])[0] == 3
            refused += 1
        else:
            assert rc == 0 and st == 0, (tag, rc, st)
    assert refused == 1 and names[[k for k in range(7) if np.isinf(z["const%d" % k]).any()][0]] == "mines:replay:91"


def test_every_fixture_reward_bit_for_bit(lib, fix):
    z, names = fix
    rows = 0
    for k, tag in enumerate(names):
        for pre, pos, flags, frames, par in rollouts(z, k):
            rc, rew, comp, kind = host_reward(lib, z["m%d" % k], pos, flags, frames, par)
            assert rc == 0, (tag, pre)
            want = z["%srew%d" % (pre, k)]
            bad = np.flatnonzero(rew.view(np.uint64) != want.view(np.uint64))
            assert len(bad) == 0, (tag, pre, len(bad), bad[:5], rew[bad[:5]], want[bad[:5]])
            assert np.array_equal(kind, z["%skind%d" % (pre, k)]), (tag, pre)
            # components: pbrs, the two milestones (the fixture's column 1 is the distance milestone on a live step and the switch
            # milestone on a terminal one), approach bonus, terminal reward
            ref = z["%scomp%d" % (pre, k)]
            live = kind != 3
            assert np.array_equal(comp[:, 0], ref[:, 0]) and np.array_equal(comp[:, 3], ref[:, 2]), (tag, pre)
            assert np.array_equal(np.where(live, comp[:, 1], comp[:, 2]), ref[:, 1]), (tag, pre)
            dead = (flags & 2) != 0
            assert np.array_equal(comp[:, 4], ref[:, 3]), (tag, pre)
            assert (comp[dead, 4] == (z["params_c"] if par is not None else z["params"])[0] + comp[dead, 2]).all()
            rows += len(want)
    assert rows > 2800


def test_state_restarts_at_episode_ends(lib, fix):
    """An episode replayed on its own, from a fresh state, gives the rewards it gave inside the long rollout: nothing of the reward
    state but the path calculator's last-call record crosses an episode end, and that record is rewritten by the spawn observation."""
    z, names = fix
    k = names.index("c0:replay:0")
    pos, flags, frames = z["apos%d" % k], z["aflags%d" % k], z["aframes%d" % k]
    _, rew, _, _ = host_reward(lib, z["m%d" % k], pos, flags, frames)
    ends = np.flatnonzero((flags & 3) != 0)
    assert len(ends) >= 5
    for a, b in zip(ends[:-1] + 1, ends[1:] + 1):
        _, part, _, kind = host_reward(lib, z["m%d" % k], pos[a:b + 1], flags[a:b], frames[a:b])
        assert np.array_equal(part, rew[a:b]) and kind[-1] == 3
    # and without auto-reset the terminal step leaves the state alone: the terminal reward comes again
    a, b = ends[0] + 1, ends[1] + 1
    _, twice, _, _ = host_reward(lib, z["m%d" % k], np.concatenate([pos[a:b], pos[b - 1:b], pos[b - 1:b]]), np.append(flags[a:b], flags[b - 1]),
                                 np.append(frames[a:b], frames[b - 1]), end_bits=0)
    assert twice[-1] == twice[-2] == rew[b - 1]


def test_refused_levels(lib, fix):
    """Several exit switches (npp_reachability refuses them) and a map that does not compile."""
    z, names = fix
    m = np.array(z["m%d" % names.index("c0:replay:0")], dtype=np.float64)
    assert int(m[1156]) == 1   # one exit door; its record is the first entity (type 3), the switch (type 4) follows
    i = 1230
    while int(m[i]) != 3:
        i += 9 if int(m[i]) in (6, 8) else 5
    two = np.concatenate([m[:i], m[i:i + 5], m[i:i + 5] + [0, 8, 0, 0, 0], m[i + 5:i + 10], m[i + 5:i + 10] + [0, 8, 0, 0, 0], m[i + 10:]])
    two[1156] = 2
    from nclone_amd.engine import reach_level_info

    assert not reach_level_info(two)["supported"]
    rc, out, st = level_constants(lib, two)
    assert rc == 3 and st == 2 and np.isinf(out).all()
    assert host_reward(lib, two, np.zeros((1, 2)), [], [])[0] == 3
    assert level_constants(lib, m[:100])[0] == 1   # NPP_ERR_INVALID


def test_potential_and_approach_bonus_grids(lib, fix):
    """The two RewardConfig-independent pieces against the reference's own functions, called directly by the generator:
    objective_distance_potential on distances around k, 0 and inf in both phases, _calculate_completion_approach_bonus around 100.
    They are reached through npp_reward_host on a level of the fixture by choosing what the rule cannot tell from a rollout --
    here they are compiled from the header itself."""
    z, _ = fix
    src = open(os.path.join(ROOT, "nclone_amd", "csrc", "npp_reward.hpp")).read()
    assert "REWARD_APPROACH_MAX * (r * r)" in src   # the product the grid below pins against the reference's `** 2`
    import subprocess
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        cpp = os.path.join(d, "grid.cpp")
        with open(cpp, "w") as f:
            f.write('#include <cstdio>\n#include <cstring>\n#include <cstdint>\n#include "npp_reward.hpp"\n'
                    "using namespace npp;\n"
                    "int main() { double v[7]; char tag; while (std::scanf(\" %c\", &tag) == 1) { double r = 0;\n"
                    "  if (tag == 'a') { std::scanf(\"%la\", &v[0]); r = reward_approach_bonus(v[0]); }\n"
                    "  else { for (int i = 0; i < 6; i++) std::scanf(\"%la\", &v[i]);\n"
                    "         r = reward_objective_potential(v[0], (int)v[1], v[2], v[3], v[4], v[5]); }\n"
                    "  std::printf(\"%a\\n\", r); } return 0; }\n")
        exe = os.path.join(d, "grid")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "nclone_amd", "csrc"),
                               "-I", os.path.join(ROOT, "include"), cpp, "-o", exe])
        lines = ["a %s" % float(x).hex() for x in z["app_in"]]
        for s2s, s2e, sw, dist, px, py, sx, sy, ex, ey in z["pot_in"]:
            gx, gy = (ex, ey) if sw else (sx, sy)
            lines.append("p " + " ".join(float(x).hex() for x in (dist, sw, s2s, s2e, int(gx) - int(px), int(gy) - int(py))))
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split()
    got = np.array([float.fromhex(x) for x in out])
    na = len(z["app_in"])
    app, pot = got[:na], got[na:]
    assert np.array_equal(pot.view(np.uint64), z["pot_out"].view(np.uint64)), np.flatnonzero(pot != z["pot_out"])
    differ = np.flatnonzero(app.view(np.uint64) != z["app_out"].view(np.uint64))
    assert len(differ) == 0, (len(differ), z["app_in"][differ[:5]], app[differ[:5]], z["app_out"][differ[:5]])
    assert z["app_none"][0] == 0.0


def test_truncation_branch(lib, fix):
    """A step that ends by truncation under auto-reset (flags bit 3 in end_bits): the known deviation -- time penalty times frames
    plus the switch milestone, times 0.1, no shaping term -- and the state restarts as at any episode end."""
    z, names = fix
    k = names.index("mines:replay:24")
    pos, flags, frames = z["apos%d" % k][:31].copy(), z["aflags%d" % k][:30].copy(), z["aframes%d" % k][:30].copy()
    assert not (flags[:12] & 3).any()
    flags[10] |= 8
    pos[11:] = z["apos%d" % k][:20]   # the env is back at its spawn and plays the rollout's first steps again
    flags[11:], frames[11:] = z["aflags%d" % k][:19], z["aframes%d" % k][:19]
    par = z["params_c"]
    rc, rew, comp, kind = host_reward(lib, z["m%d" % k], pos, flags, frames, par, end_bits=11)
    assert rc == 0 and kind[10] == 3 and not comp[10].any()
    assert rew[10] == (par[3] * float(frames[10])) * 0.1 and rew[10] < 0
    _, first, comp1, _ = host_reward(lib, z["m%d" % k], z["apos%d" % k][:20], z["aflags%d" % k][:19], z["aframes%d" % k][:19], par, end_bits=11)
    assert np.array_equal(rew[11:], first) and comp[11, 0] == 0.0   # a fresh episode


def test_host_entries_under_asan_and_ubsan(fix, tmp_path):
    """npp_reward_level_constants_host and npp_reward_host in a stand-alone program (tests/reward_sanitized_main.cpp) built with
    g++ -fsanitize=address,undefined together with the host sources, runtimes linked statically: on a fixture rollout it must print the fixture's
    constants and rewards, on truncated and lying maps it must refuse, and no sanitizer report may appear."""
    import subprocess

    from nclone_amd import build_native

    z, names = fix
    # ONE executable: the driver and the host sources, with the sanitizer runtimes linked statically, so that it stands alone whatever
    # the environment it is started in holds (no dynamic runtime, hence no link-order requirement; the environment is passed on as it is)
    exe = str(tmp_path / "reward_sanitized_main")
    srcs = [os.path.join(build_native.CSRC, f) for f in build_native.HOST_SOURCES]
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-static-libasan",
                        "-static-libubsan", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "reward_sanitized_main.cpp")] + srcs + ["-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=23", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for tag, pre in (("c0:replay:20", "a"), ("mines:replay:24", "d"), ("mines:replay:91", None)):
        k = names.index(tag)
        src = pre or "a"
        if pre is None:   # the level the reference raises on: a refusal, with rollout rows of another level as filler
            pos, flags, frames = z["apos0"][:9], z["aflags0"][:8], z["aframes0"][:8]
        else:
            pos, flags, frames = z["%spos%d" % (src, k)], z["%sflags%d" % (src, k)], z["%sframes%d" % (src, k)]
        files = {}
        for name, a, dt in (("map", z["m%d" % k], np.float64), ("pos", pos, np.float64), ("flags", flags, np.uint8), ("frames", frames, np.uint16)):
            files[name] = str(tmp_path / (name + ".bin"))
            np.ascontiguousarray(a, dtype=dt).tofile(files[name])
        r = subprocess.run([exe, files["map"], files["pos"], files["flags"], files["frames"], str(len(flags)), str(END_BITS)],
                           capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, (tag, r.returncode, r.stdout[-500:], r.stderr[-3000:])
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
        out = r.stdout.split("\n")
        head = out[0].split()
        got_c = np.array([float.fromhex(x) if "inf" not in x else float(x) for x in head[3:6]])
        assert np.array_equal(got_c, z["const%d" % k]), (tag, out[0])
        if pre is None:
            assert head[1:3] == ["3", "2"] and out[1] == "rewards 3"
        else:
            assert head[1:3] == ["0", "0"] and out[1] == "rewards 0"
            rows = [l.split() for l in out[2:2 + len(flags)]]
            rew = np.array([float.fromhex(a) for a, _ in rows])
            assert np.array_equal(rew.view(np.uint64), z["%srew%d" % (pre, k)].view(np.uint64)), tag
            assert np.array_equal(np.array([int(b) for _, b in rows]), z["%skind%d" % (pre, k)]), tag
        assert int(out[-2].split()[-1]) >= 30, out[-2]   # the malformed maps were refused


def test_header_declares_the_entry_points():
    h = open(os.path.join(ROOT, "include", "npp_amd.h")).read()
    for name in ("npp_set_reward_mode", "npp_set_reward_params", "npp_step_reward", "npp_reward_host", "npp_reward_level_constants_host",
                 "npp_reward_default_params"):
        assert re.search(r"\b%s\(" % name, h), name
    assert "sparse mode: none; pbrs mode:" in h
