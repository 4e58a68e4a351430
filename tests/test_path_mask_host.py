"""CPU checks of path-direction action masking (include/npp_amd.h npp_set_action_masking): the detector the device
kernel runs (npp_pathmask.hpp, through npp_path_direction_host) against tests/golden/pathmask.npz -- directions and from-graph
bits produced by running the reference's _detect_straight_path_direction on rollouts and off-trajectory probes --, the keep-masks
against the reference's hard masks, and the C ABI surface."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.path_mask_ref import KEEP, hard_mask_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS = ("pos", "sw", "inert", "dir", "hard", "graph")


@pytest.fixture(scope="module")
def lib():
    from nclone_amd import build_native

    build_native.build()
    from nclone_amd import _native

    return _native.lib()


@pytest.fixture(scope="module")
def fix():
    z = np.load(os.path.join(ROOT, "tests", "golden", "pathmask.npz"))
    return z, bytes(z["names"]).decode().split("\n")


def host_direction(lib, m, pos, sw):
    m = np.ascontiguousarray(m, dtype=np.float64)
    pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 2)
    sw = np.ascontiguousarray(sw, dtype=np.uint8)
    assert len(sw) == len(pos)
    d = np.full(len(pos), -1, dtype=np.int8)
    g = np.full(len(pos), 255, dtype=np.uint8)
    st = np.full(1, -1, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.npp_path_direction_host(m.ctypes.data_as(C.POINTER(C.c_double)), m.size, p(pos), p(sw), len(pos), p(d), p(g), p(st)) == 0
    assert st[0] == 0
    return d, g


def rollout_rows(z, k):
    """every rollout row of level k: both rollouts, the returned observations and the terminal ones"""
    return {c: np.concatenate([z["%s%s%d" % (pre, c, k)] for pre in ("a", "at", "b", "bt")]) for c in COLS}


def lattice(z):
    x0, y0, step, nx, ny = z["lat"]
    lx, ly = x0 + step * np.arange(int(nx)), y0 + step * np.arange(int(ny))
    return np.stack(np.meshgrid(lx, ly, indexing="ij"), axis=-1).reshape(-1, 2)


def test_fixture_covers_every_branch(lib, fix):
    z, names = fix
    assert len(names) == 7 and "doors:replay:127" in names
    probe, roll = np.zeros((2, 4), int), np.zeros((2, 4), int)
    for k in range(len(names)):
        for s in (0, 1):
            probe[s] += np.bincount(np.concatenate([z["latdir%d" % k][s].ravel(), z["pdir%d" % k][s]]), minlength=4)
        r = rollout_rows(z, k)
        for s in (0, 1):
            roll[s] += np.bincount(r["dir"][r["sw"] == s], minlength=4)
    assert (probe >= 50).all(), probe
    assert (roll[:, 1] + roll[:, 2] >= 1).all() and (roll[:, 3] >= 1).all(), roll
    # doors:replay:127 (switch 6 px from its door): the replay reaches the exit phase.  No trajectory row of the file lies in the
    # near-goal branch, and none can: the ninja collects the switch at 16 px and enters the door at 22 px, both beyond the 12 px
    # of STRAIGHT_PATH_MIN_DISTANCE -- the branch is pinned by the probes (rings around both goals) alone.
    k = names.index("doors:replay:127")
    assert z["bsw%d" % k][-2] == 1 and z["bterm%d" % k][-1] == 1
    m = np.ascontiguousarray(z["m%d" % k], dtype=np.float64)
    info = np.zeros(14, dtype=np.int32)
    assert lib.npp_reach_compile(m.ctypes.data_as(C.POINTER(C.c_double)), m.size, info.ctypes.data_as(C.c_void_p), *([None] * 11)) == 0
    near = 0
    for s in (0, 1):
        d = ((info[6 + 2 * s:8 + 2 * s][None, :] - z["ppos%d" % k]) ** 2).sum(axis=1) ** 0.5
        assert not z["pgraph%d" % k][s][d < 12.0].any()
        near += len(set(z["pdir%d" % k][s][d < 12.0].tolist()) & {0, 1, 2})
    assert near == 6   # none, left and right under both goals


def test_host_detector_matches_reference_on_every_row(lib, fix):
    """No row left out: rollout rows (returned and terminal observations of both rollouts), the probe lattice and the special
    probes under both switch bits.  Directions and from-graph bits are integers: equal or not."""
    z, names = fix
    lat = lattice(z)
    rows = 0
    for k, name in enumerate(names):
        m = z["m%d" % k]
        r = rollout_rows(z, k)
        d, g = host_direction(lib, m, r["pos"], r["sw"])
        bad = np.flatnonzero((d != r["dir"]) | (g != r["graph"]))
        assert len(bad) == 0, (name, "rollout", bad[:5], r["pos"][bad[:5]], d[bad[:5]], r["dir"][bad[:5]])
        rows += len(d)
        for pts, dk, gk in ((lat, z["latdir%d" % k].reshape(2, -1), z["latgraph%d" % k].reshape(2, -1)),
                            (z["ppos%d" % k], z["pdir%d" % k], z["pgraph%d" % k])):
            for s in (0, 1):
                d, g = host_direction(lib, m, pts, np.full(len(pts), s, dtype=np.uint8))
                bad = np.flatnonzero((d != dk[s]) | (g != gk[s]))
                assert len(bad) == 0, (name, "probe", s, bad[:5], pts[bad[:5]], d[bad[:5]], dk[s][bad[:5]])
                rows += len(d)
    assert rows > 570000


def test_keep_masks_give_the_reference_hard_mask(fix):
    z, names = fix
    seen = set()
    for k in range(len(names)):
        r = rollout_rows(z, k)
        assert np.array_equal(hard_mask_bits(r["inert"], r["dir"]), r["hard"]), names[k]
        assert (r["hard"] & 1).all()   # nothing ever clears NOOP: the "unmask NOOP if empty" rule cannot fire
        seen |= set(np.unique(r["dir"][r["hard"] != r["inert"]]).tolist())
    assert seen == {1, 2, 3}   # every direction removed something somewhere


def test_header_constants_equal_the_python_keep_masks():
    src = open(os.path.join(ROOT, "nclone_amd", "csrc", "npp_pathmask.hpp")).read()
    for d, name in enumerate(("NONE", "LEFT", "RIGHT", "DOWN")):
        mt = re.search(r"PATH_KEEP_%s = (0x[0-9a-f]+);" % name, src)
        assert mt and int(mt.group(1), 16) == int(KEEP[d]), name
        assert re.search(r"PATH_%s = %d\b" % (name, d), src), name
    assert "PATH_KEEP_NONE | (PATH_KEEP_LEFT << 8) | (PATH_KEEP_RIGHT << 16) | (PATH_KEEP_DOWN << 24)" in src


def test_abi_surface(lib):
    from nclone_amd import _native as nat

    new = ("npp_set_action_masking", "npp_path_action_mask", "npp_path_mask_stats_view", "npp_path_direction_host")
    for name in new:
        assert name in nat.EXPORTS and getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int, name
    assert lib.npp_set_action_masking(None, 1) == nat.NPP_ERR_INVALID
    assert lib.npp_path_action_mask(None, None, None, None) == nat.NPP_ERR_INVALID
    assert lib.npp_path_mask_stats_view(None, None, None, None, None) == nat.NPP_ERR_INVALID
    assert lib.npp_path_direction_host(None, 0, None, None, 0, None, None, None) == nat.NPP_ERR_INVALID
    hdr = open(os.path.join(ROOT, "include", "npp_amd.h")).read()
    for cite in ("base_environment.py:3050", "3075-3107", ":3109-3253", "ninja.py:743-800", "nsim.py:48", "reward_config.py:815-865",
                 "pathfinding_utils.py:1331-1496", "path_distance_cache.py:162-185"):
        assert cite in hdr, cite


def test_python_surface_refuses_what_it_documents():
    """The classes that cannot serve the option say so (no GPU needed: the checks come first)."""
    from nclone_amd.async_env import NppAsyncVecEnvironment
    from nclone_amd.vec_env import NppVecEnvironment

    with pytest.raises(ValueError, match="action masking"):
        NppAsyncVecEnvironment([], 4, action_masking_mode="hard")
    with pytest.raises(ValueError, match="action_masking_mode"):
        NppVecEnvironment([], 4, action_masking_mode="medium")
