"""CPU checks of the minimal observation mode (the reference's observation_mode = MINIMAL): the observation space, the argument
checks of the host classes (raised before any handle is created: no device needed), the ABI symbols, and the coverage of the
fixture tests/golden/minimal.npz (produced by running the reference, tests/golden/make_golden_minimal.py)."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFLICTS = ("enable_visual_observations", "enable_visual_frame_stacking", "enable_state_stacking", "enable_graph_observations",
             "enable_spatial_context", "enable_reachability", "enable_switch_states")


def test_minimal_observation_space():
    """Exactly the reference's two-key Dict (npp_environment.py:211-231)."""
    from nclone_amd import spaces

    for kw in ({}, {"visual": True, "reachability": True, "state_stack": 4, "graph": True}):
        s = spaces.observation_space(minimal=True, **kw)
        assert list(s.spaces.keys()) == ["minimal_observation", "action_mask"]
        m, a = s["minimal_observation"], s["action_mask"]
        assert tuple(m.shape) == (40,) and m.dtype == np.float32 and np.all(m.low == -1.0) and np.all(m.high == 1.0)
        assert tuple(a.shape) == (6,) and a.dtype == np.int8 and np.all(a.low == 0) and np.all(a.high == 1)
    assert "minimal_observation" not in spaces.observation_space().spaces and "game_state" in spaces.observation_space().spaces


def _no_device(monkeypatch):
    """Any attempt to create a handle fails the test: the checks below must raise before that."""
    from nclone_amd import engine

    def boom(*a, **k):
        raise AssertionError("a handle was created before the arguments were checked")

    monkeypatch.setattr(engine.NppBatch, "__init__", boom)


@pytest.mark.parametrize("option", CONFLICTS)
def test_conflicting_options_raise_before_the_handle(monkeypatch, option):
    from nclone_amd.vec_env import NppEnvironment, NppVecEnvironment

    _no_device(monkeypatch)
    lv = [np.zeros(1245)]
    with pytest.raises(ValueError, match=option):
        NppVecEnvironment(lv, 4, observation_mode="minimal", **{option: True})
    with pytest.raises(ValueError, match=option):
        NppEnvironment(map_data=lv[0], observation_mode="minimal", **{option: True})


def test_unknown_mode_raises_and_async_env_refuses(monkeypatch):
    from nclone_amd.async_env import NppAsyncVecEnvironment
    from nclone_amd.vec_env import NppEnvironment, NppVecEnvironment

    _no_device(monkeypatch)
    lv = [np.zeros(1245)]
    for mode in ("MINIMAL", "small", None, 1):
        with pytest.raises(ValueError, match="observation_mode"):
            NppVecEnvironment(lv, 4, observation_mode=mode)
        with pytest.raises(ValueError, match="observation_mode"):
            NppEnvironment(map_data=lv[0], observation_mode=mode)
    with pytest.raises(NotImplementedError, match="observation_mode"):
        NppAsyncVecEnvironment(lv, 4, n_streams=2, observation_mode="minimal")


def test_abi_symbols_and_argtypes():
    from nclone_amd import _native as nat
    from nclone_amd import build_native

    build_native.build()
    lib = nat.lib()
    assert {"npp_set_minimal_observation", "npp_minimal_observation"} <= set(nat.EXPORTS)
    assert lib.npp_minimal_observation.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p] and lib.npp_minimal_observation.restype == C.c_int
    assert lib.npp_set_minimal_observation.argtypes == [C.c_void_p, C.c_int] and lib.npp_set_minimal_observation.restype == C.c_int
    assert nat.MINIMAL_OBS_DIM == 40
    hdr = open(os.path.join(ROOT, "include", "npp_amd.h")).read()
    assert "#define NPP_MINIMAL_OBS_DIM 40" in hdr
    assert "int npp_minimal_observation(npp_handle h, float *d_out /* [N,40] */, int32_t *d_status /* [N] or NULL */);" in hdr
    # NULL handle / NULL output are bad arguments, not crashes (no device is touched)
    assert lib.npp_minimal_observation(None, None, None) == nat.NPP_ERR_INVALID
    assert lib.npp_set_minimal_observation(None, 1) == nat.NPP_ERR_INVALID
    from nclone_amd import engine

    assert engine._FIELDS["minimal_observation"][0] == (40,) and "minimal_observation" in engine._OPTIONAL
    assert list(engine._FIELDS)[:7] == ["game_state", "entity_pos", "reward", "frames", "action_mask", "flags", "terminal_state"]   # packed block untouched


def test_fixture_coverage():
    """What make_golden_minimal.py prints, re-asserted from the file.  Columns 14, 15 (waypoint direction) and 18 (phase) are
    identically 0 in everything the reference produces when run this way: asserted as exact zeros.  Column 39 (launch pad buffer)
    is -1 in every row: no plan the generator tried (see its docstring) leaves the buffer set at an observation; asserted as such,
    so that a regenerated fixture which does reach it is noticed and the exemption removed.  The column's other values are pinned
    by test_state_encodings_match_numpy_on_every_field_value below."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "minimal.npz"))
    names = bytes(z["names"]).decode().split("\n")
    n = len(names)
    assert sum(t.startswith("doors:") for t in names) >= 1 and sum(t.startswith("mines:") for t in names) >= 1
    assert sum(t.startswith("zoo:") for t in names) >= 1
    reach = set(bytes(np.load(os.path.join(ROOT, "tests", "golden", "reach.npz"))["names"]).decode().split("\n"))
    reach |= set(bytes(np.load(os.path.join(ROOT, "tests", "golden", "reach2.npz"))["names"]).decode().split("\n"))
    assert set(names) <= reach   # the reachability side is pinned on every level
    rows = np.concatenate([z["o%d" % k] for k in range(n)] + [z["ot%d" % k] for k in range(n)])
    assert rows.dtype == np.float32 and rows.shape[1] == 40
    for k in range(n):
        steps = len(z["a%d" % k])
        assert z["o%d" % k].shape == (steps + 1, 40) and z["rf%d" % k].shape == (steps + 1, 38) and z["sc%d" % k].shape == (steps + 1, 48)
        assert z["ot%d" % k].shape == (int(z["t%d" % k].sum()), 40)
        # the rows are what their recorded inputs say (reachability and mine columns are plain copies)
        assert np.array_equal(z["o%d" % k][:, 12:20], z["rf%d" % k][:, [13, 14, 15, 16, 8, 9, 12, 24]])
        assert np.array_equal(z["o%d" % k][:, 20:36], z["sc%d" % k].reshape(-1, 8, 6)[:, :4][:, :, [0, 1, 2, 5]].reshape(-1, 16))
    distinct = [len(np.unique(rows[:, c])) for c in range(40)]
    for c in range(40):
        if c in (14, 15, 18):
            assert (rows[:, c] == 0).all(), c
        elif c == 39:
            assert (rows[:, c] == -1).all()
        else:
            assert distinct[c] >= 2, (c, distinct)
    # at least four toggle mines within range somewhere (the fourth mine's columns vary), and a capped state (dead ninja)
    assert (np.abs(rows[:, 32:34]).sum(axis=1) > 0).sum() > 100
    capped = sum(int((z["stt%d" % k] > 4).sum()) for k in range(n))
    assert capped >= 1
    for k in range(n):
        dead = z["stt%d" % k] > 4
        assert (z["ot%d" % k][dead][:, 6] == 1).all() and not z["ot%d" % k][dead][:, 2:6].any()
    assert np.isfinite(rows).all()   # (the reference does not clip: yspeed / MAX_HOR_SPEED leaves the declared [-1, 1])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "minimal.npz")) < 1024 * 1024


def test_state_encodings_match_numpy_on_every_field_value():
    """npp_minimal_encode_host runs the function the device kernel runs (npp_minimal.hpp compiles for both): columns 0-11 and
    36-39 against the reference's formulas in numpy f64 with one rounding to f32, for every state code, flag, wall normal and
    EVERY buffer value -1 .. 5 of all four buffers -- including the non-negative launch-pad values (column 39, span 4) that no
    reference rollout of the fixtures reaches -- and velocities / floor normals of a seeded random draw."""
    from nclone_amd import _native as nat
    from nclone_amd import build_native

    build_native.build()
    lib = nat.lib()
    rng = np.random.default_rng(5)
    words, planes = [], []
    for state in range(10):
        for airborn in (0, 1):
            for walled in (0, 1):
                for wn in (-1, 0, 1):
                    for buf in range(-1, 6):
                        for which in range(4):
                            b = [int(rng.integers(-1, 6)) for _ in range(4)]
                            b[which] = buf
                            words.append(state | airborn << 4 | walled << 6 | (wn + 1) << 7 | (b[0] + 1) << 15 | (b[1] + 1) << 18
                                         | (b[2] + 1) << 21 | (b[3] + 1) << 24 | int(rng.integers(0, 4)) << 27)
                            planes.append([rng.normal() * 3, rng.normal() * 3, rng.uniform(-1, 1), rng.uniform(-1, 1)])
    A = np.array(words, dtype=np.uint32)
    P = np.ascontiguousarray(planes, dtype=np.float64)
    P[:7] = [[0.0, -0.0, 0.0, -1.0], [3.333, -3.333, 1.0, 0.0], [1e-300, 5.0, -0.0, -0.0], [10.0, -10.0, 0.6, -0.8],
             [3.3329999999999997, 1 / 3, 2 ** -0.5, -(2 ** -0.5)], [0.1, 0.2, 0.3, 0.4], [-6.0, 6.0, -1.0, 1.0]]
    n = len(A)
    got = np.full((n, 40), 7.0, dtype=np.float32)
    assert lib.npp_minimal_encode_host(A.ctypes.data, P.ctypes.data, n, got.ctypes.data) == nat.NPP_OK
    want = np.full((n, 40), 7.0, dtype=np.float32)
    state = (A & 15).astype(np.int64)
    walled = (A >> 6) & 1
    want[:, 0] = P[:, 0] / 3.333   # MAX_HOR_SPEED
    want[:, 1] = P[:, 1] / 3.333
    want[:, 2:7] = 0.0
    want[np.arange(n), 2 + np.minimum(state, 4)] = 1.0
    want[:, 7] = np.where((A >> 4) & 1, 1.0, -1.0)
    want[:, 8] = np.where(walled, 1.0, -1.0)
    want[:, 9] = np.where(walled, ((A >> 7) & 3).astype(np.float64) - 1.0, 0.0)
    want[:, 10] = P[:, 2]
    want[:, 11] = P[:, 3]
    for c, shift, span in ((36, 15, 5.0), (37, 18, 5.0), (38, 21, 5.0), (39, 24, 4.0)):
        buf = ((A >> shift) & 7).astype(np.float64) - 1.0
        want[:, c] = np.where(buf >= 0, buf / span, -1.0)
    assert set(np.unique(want[:, 39]).tolist()) == {-1.0, 0.0, 0.25, 0.5, 0.75, 1.0, 1.25}
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))   # bit for bit; columns 12-35 untouched (still 7.0)
    assert lib.npp_minimal_encode_host(None, None, 3, None) == nat.NPP_ERR_INVALID
