"""Host-side tests of the action routes (include/npp_amd.h npp_set_routes): the C entries are declared, exported and
bound; npp_route_apply_host -- the rule the device kernels compile (csrc/npp_route.hpp) -- equals the Python model
(tests/route_ref.py) on seeded event lists; every checkpoint of the reference fixture (tests/golden/routes.npz) is reached by the
oracle replaying its route from the spawn; route_to_replay round-trips through the replay format; the argument checks of the host
classes that need no device.  The kernels are tested in tests/test_gpu_routes.py."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import route_ref as ref

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"npp_set_routes": 2, "npp_route_view": 4, "npp_archive_route_view": 4, "npp_route_apply_host": 7}


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_entries_declared_exported_and_bound():
    from nclone_amd import _native as nat

    hdr = open(os.path.join(ROOT, "include", "npp_amd.h")).read()
    lib = nat.lib()
    for name, argc in ENTRIES.items():
        assert "int %s(" % name in hdr, name
        assert name in nat.EXPORTS, name
        fn = getattr(lib, name)   # AttributeError when the library does not export it
        assert fn.argtypes is not None and len(fn.argtypes) == argc and fn.restype is C.c_int, name
    for cite in ("state_checkpoint.py", "base_environment.py:186", ":517", ":1677", ":2114", ":2332-2349"):
        assert cite in hdr, cite
    # without a handle the entries answer instead of crashing
    assert lib.npp_set_routes(None, 64) == nat.NPP_ERR_INVALID
    assert lib.npp_route_view(None, None, None, None) == nat.NPP_ERR_INVALID
    assert lib.npp_archive_route_view(None, None, None, None) == nat.NPP_ERR_INVALID
    assert lib.npp_route_apply_host(None, None, 16, 0, None, 0, None) == nat.NPP_ERR_INVALID
    h, a = np.zeros(16, dtype=np.int32), np.zeros((2, 16), dtype=np.uint8)
    assert lib.npp_route_apply_host(_ptr(h), _ptr(a), 24, 0, None, 0, None) == nat.NPP_ERR_INVALID   # not a multiple of 16
    bad = np.array([[9, 0, 0, 0, 0, 0, 0, 0]], dtype=np.int32)
    assert lib.npp_route_apply_host(_ptr(h), _ptr(a), 16, 0, _ptr(bad), 1, None) == nat.NPP_ERR_INVALID


def _apply_native(lib, route, events, pool):
    hdr = np.array(route.hdr, dtype=np.int32)
    buf = route.buf.copy()
    ev = np.ascontiguousarray(events, dtype=np.int32)
    rc = lib.npp_route_apply_host(_ptr(hdr), _ptr(buf), route.cap, 1 if route.autoreset else 0, _ptr(ev), len(ev), _ptr(pool))
    assert rc == 0, lib.npp_last_error(None)
    return hdr, buf


def test_apply_host_equals_the_model_on_random_event_lists():
    """200 seeded lists; over all of them every branch of the rule is taken (asserted below): steps that execute no frame,
    episode ends with and without auto-reset, resets of empty routes, overflow at cap = 16, a frame_skip change, a tick, a restore."""
    from nclone_amd import _native as nat

    lib = nat.lib()
    seen = {"x0": 0, "end_auto": 0, "end_manual": 0, "reset_empty": 0, "overflow": 0, "fs_change": 0, "tick": 0, "restore": 0}
    for seed in range(200):
        rng = np.random.default_rng(9000 + seed)
        cap = 16 if seed % 2 == 0 else int(rng.choice([32, 64]))
        auto = seed % 4 < 2
        pool = rng.integers(0, 6, size=4 * 64 + cap, dtype=np.uint8)
        events = ref.random_events(rng, cap, int(rng.integers(20, 120)), pool)
        model = ref.Route(cap, auto)
        native = ref.Route(cap, auto)   # (carries the native state from event to event)
        for ev in events:   # event by event: the branch bookkeeping reads the model's state before each one
            if ev[0] == 0:
                seen["x0"] += ev[3] == 0
                if ev[3] > 0 and not model.empty() and model.hdr[ref.FS] != ev[4]:
                    seen["fs_change"] += 1
                if ev[3] > 0 and model.hdr[ref.LEN] == cap:
                    seen["overflow"] += 1
                if ev[2] & ref.END:
                    seen["end_auto" if auto else "end_manual"] += 1
            elif ev[0] == 1:
                seen["reset_empty"] += model.empty()
            elif ev[0] == 2:
                seen["tick"] += 1
            else:
                seen["restore"] += 1
            ref.apply_events(model, [ev], pool)
            hdr, buf = _apply_native(lib, native, [ev], pool)
            native.hdr, native.buf = [int(v) for v in hdr], buf
            assert native.hdr == model.hdr, (seed, ev, native.hdr, model.hdr)
            assert np.array_equal(native.buf, model.buf), (seed, ev)
        # and the whole list in one call
        hdr, buf = _apply_native(lib, ref.Route(cap, auto), events, pool)
        assert [int(v) for v in hdr] == model.hdr and np.array_equal(buf, model.buf), seed
        assert model.hdr[13:] == [0, 0, 0] and model.hdr[ref.CUR] in (0, 1)
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("variant", ["pow", "mul"])
def test_fixture_checkpoints_are_reached_by_the_oracle(golden, oracle_mod, variant):
    """Each checkpoint of routes.npz (the reference's StateCheckpoint, accepted by the reference's ActionReplayer) replayed from
    the spawn by the oracle: position and velocity as test_oracle_golden.py compares reference fixtures (bit for bit; `mul` on the
    entity-zoo level within 1e-5 px, as test_oracle_zoo_replays allows), frame count and switch state equal."""
    r = golden.z("routes")
    names = golden.names("routes")
    assert len(names) == 5
    total = late = 0
    for k, name in enumerate(names):
        plan, marks = r["a%d" % k], r["t%d" % k]
        assert int(marks.sum()) >= 2, name
        first_end = int(np.flatnonzero(marks)[0]) + 1
        for c, (cs, cl) in enumerate(zip(r["cs%d" % k], r["cl%d" % k])):
            route = plan[cs - cl:cs]
            assert cl > 0 and not marks[cs - cl:cs].any() and (cs == cl or marks[cs - cl - 1]), (name, c)
            o = oracle_mod.Oracle(variant)
            assert o.load(r["m%d" % k]) == 0
            for a in route:
                ex, fl = o.env_step(int(a), 4)
                assert ex == 4 and fl == 0, (name, c)
            f, d = o.core()
            want = np.concatenate([r["cp%d" % k][c], r["cv%d" % k][c]])
            if variant == "pow" or not name.startswith("zoo:"):
                assert np.array_equal(f[:4], want), (name, c, f[:4], want)
            else:
                assert np.abs(f[:4] - want).max() <= 1e-5, (name, c, f[:4], want)
            assert o.frame == int(r["cf%d" % k][c]) == 4 * cl, (name, c)
            assert (d[13] != 1) == bool(r["cw%d" % k][c]), (name, c)
            total += 1
            late += cs > first_end
    assert total >= 60 and late >= 8


def test_route_to_replay_round_trip():
    from nclone_amd.replay import CompactReplay, decode_input_to_controls, route_to_replay
    from nclone_amd.vec_env import ACTION_TABLE

    rng = np.random.default_rng(5)
    m = rng.integers(0, 256, size=1335, dtype=np.uint8)
    actions = np.concatenate([np.arange(6), rng.integers(0, 6, size=40)]).astype(np.uint8)
    for fs in (1, 4):
        for success in (True, False):
            rep = route_to_replay(m, actions, fs, success)
            back = CompactReplay.from_binary(rep.to_binary())
            assert back.map_data == m.tobytes() and back.success is success and back.version == 1
            assert len(back.input_sequence) == fs * len(actions)
            for i, b in enumerate(back.input_sequence):
                assert decode_input_to_controls(b) == ACTION_TABLE[actions[i // fs]], (fs, i)
    assert route_to_replay(bytes(m), [], 4, True).input_sequence == []
    with pytest.raises(ValueError, match="frame_skip"):
        route_to_replay(m, actions, 0, True)
    with pytest.raises(ValueError, match="not in 0..5"):
        route_to_replay(m, [0, 6], 4, True)


def test_argument_checks_need_no_device():
    from nclone_amd.vec_env import NppEnvironment, NppVecEnvironment, route_capacity_for

    # the default capacity: the longest episode the env can have
    assert route_capacity_for(False, None, 4, "dynamic") == 0
    assert route_capacity_for(True, None, 4, "dynamic") == 2500
    assert route_capacity_for(True, None, 4, 1201) == 301
    assert route_capacity_for(True, None, 1, np.array([500, 800])) == 800
    assert route_capacity_for(True, 64, 4, "dynamic") == 64
    lvl = [np.zeros(1)]
    with pytest.raises(ValueError, match="route_capacity without record_routes"):
        NppVecEnvironment(lvl, 64, route_capacity=64)
    with pytest.raises(ValueError, match="route_capacity must be a positive"):
        NppVecEnvironment(lvl, 64, record_routes=True, route_capacity=0)
    with pytest.raises(ValueError, match="route_capacity must be a positive"):
        NppEnvironment(map_data=lvl[0], record_routes=True, route_capacity=-3)
    # record_routes needs no archive: its refusals are about the methods that read one
    v = object.__new__(NppVecEnvironment)
    v.route_capacity, v.checkpoint_slots = 64, 0
    with pytest.raises(RuntimeError, match="archive_routes: this env was created without checkpoint_slots"):
        v.archive_routes([0])
    v.route_capacity, v.checkpoint_slots = 0, 8
    for call in (lambda: v.archive_routes([0]), v.finished_routes, v.get_action_sequence_length, lambda: v.get_current_action_sequence(0)):
        with pytest.raises(RuntimeError, match="created without record_routes"):
            call()
