"""Host-side tests of the episode statistics (include/npp_amd.h npp_set_episode_stats): the C entries are declared,
exported, bound and cite the reference; npp_episode_apply_host -- the rule the device kernels compile (csrc/npp_episode.hpp) --
equals the Python model (tests/episode_ref.py) on seeded event lists, bit for bit; the fixed-point return column at its rounding
ties, at negative returns and at the clamp; the host entry under ASan + UBSan in a stand-alone program; the argument checks of the
host classes that need no device.  The kernels are tested in tests/test_gpu_episode.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import episode_ref as ref

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"npp_set_episode_stats": 2, "npp_episode_accumulate": 7, "npp_episode_restart": 3, "npp_episode_view": 4,
           "npp_episode_table_reset": 1, "npp_episode_apply_host": 9}


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_entries_declared_exported_bound_and_cited():
    from nclone_amd import _native as nat
    from nclone_amd import build_native

    hdr = open(os.path.join(ROOT, "include", "npp_amd.h")).read()
    lib = nat.lib()
    for name, argc in ENTRIES.items():
        assert "int %s(" % name in hdr, name
        assert name in nat.EXPORTS, name
        fn = getattr(lib, name)   # AttributeError when the library does not export it
        assert fn.argtypes is not None and len(fn.argtypes) == argc and fn.restype is C.c_int, name
    for cite in ("base_environment.py:1163-1242", ":156", ":676", "npp_environment.py:587", ":688", ":546-552",
                 "main_reward_calculator.py:2825-2914"):
        assert cite in hdr, cite
    assert "npp_episode.hip" in build_native.SOURCES and "npp_episode.hpp" in build_native.HEADERS
    # the header's plane and column numbers are the model's
    for name, want in (("NPP_EP_FIN = ", ref.FIN), ("NPP_EP_FIN_FLAGS = ", ref.FIN_FLAGS), ("NPP_EP_N_FINISHED = ", ref.N_FINISHED),
                       ("NPP_EP_NI = ", ref.NI), ("NPP_EP_DFIN = ", ref.DFIN), ("NPP_EP_ND = ", ref.ND), ("NPP_EP_COLS = ", ref.COLS)):
        assert "%s%d" % (name, want) in hdr, name
    # without a handle the entries answer instead of crashing
    assert lib.npp_set_episode_stats(None, 1) == nat.NPP_ERR_INVALID
    assert lib.npp_episode_accumulate(None, None, None, None, None, 1, None) == nat.NPP_ERR_INVALID
    assert lib.npp_episode_restart(None, None, 0) == nat.NPP_ERR_INVALID
    assert lib.npp_episode_view(None, None, None, None) == nat.NPP_ERR_INVALID
    assert lib.npp_episode_table_reset(None) == nat.NPP_ERR_INVALID
    assert lib.npp_episode_apply_host(None, None, None, 0, 0, None, None, 0, None) == nat.NPP_ERR_INVALID
    i, d = np.zeros(ref.NI, dtype=np.int32), np.zeros(ref.ND)
    bad = np.array([[9, 0, 0, 0, 0, 0, 0, 0]], dtype=np.int32)
    row = np.zeros((1, 8), dtype=np.float32)
    assert lib.npp_episode_apply_host(_ptr(i), _ptr(d), None, 0, 0, _ptr(bad), _ptr(row), 1, None) == nat.NPP_ERR_INVALID
    assert lib.npp_episode_apply_host(_ptr(i), _ptr(d), None, 2, 0, None, None, 0, None) == nat.NPP_ERR_INVALID   # levels without a table


def _apply_native(lib, rec, table, autoreset, events, rows):
    i = np.array(rec.i, dtype=np.int32)
    d = np.array(rec.d, dtype=np.float64)
    t = np.array(table, dtype=np.uint64).reshape(len(table), ref.COLS)
    ev = np.ascontiguousarray(events, dtype=np.int32).reshape(-1, 8)
    rw = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, 8)
    ended = np.full(1, 9, dtype=np.uint8)
    rc = lib.npp_episode_apply_host(_ptr(i), _ptr(d), _ptr(t) if len(table) else None, len(table), 1 if autoreset else 0, _ptr(ev), _ptr(rw),
                                    len(ev), _ptr(ended))
    assert rc == 0, lib.npp_last_error(None)
    return i, d, t, int(ended[0])


def _same(rec, table, i, d, t):
    return ([int(v) for v in i] == rec.i and np.array_equal(d.view(np.uint64), np.array(rec.d, dtype=np.float64).view(np.uint64))
            and [[int(v) for v in r] for r in t] == table)


def test_apply_host_equals_the_model_on_random_event_lists():
    """200 seeded lists, event by event and whole; over all of them every branch of the rule is taken (asserted below)."""
    from nclone_amd import _native as nat

    lib = nat.lib()
    seen = dict.fromkeys(("x0", "end_auto", "end_manual", "closed_truncated_row", "switch_step_1", "level_change_at_end", "reset_empty",
                          "reset_running", "restore", "restored_end", "tick", "clear", "with_comps", "without_comps", "abandoned"), 0)
    for seed in range(200):
        rng = np.random.default_rng(7000 + seed)
        n_levels = int(rng.integers(1, 5))
        auto, comps = seed % 4 < 2, seed % 2 == 0
        events, rows = ref.random_events(rng, n_levels, int(rng.integers(20, 140)), comps)
        model, table = ref.Record(), ref.new_table(n_levels)
        native, ntable = ref.Record(), ref.new_table(n_levels)   # (carry the native state from event to event)
        any_end = False
        for ev, r in zip(events, rows):   # the branch bookkeeping reads the model's state before each event
            cur = model.i
            if ev[0] == ref.EV_ROW:
                live = ev[2] > 0 and not cur[ref.BITS] & ref.CLOSED
                seen["x0"] += ev[2] == 0
                seen["closed_truncated_row"] += bool(ev[2] > 0 and cur[ref.BITS] & ref.CLOSED and ev[1] & ref.F_TRUNCATED)
                seen["switch_step_1"] += bool(live and cur[ref.STEPS] == 0 and ev[1] & ref.F_SWITCH)
                seen["with_comps" if ev[4] else "without_comps"] += 1
                if live and ev[1] & ref.END:
                    seen["end_auto" if auto else "end_manual"] += 1
                    seen["level_change_at_end"] += bool(cur[ref.STEPS] > 0 and cur[ref.LEVEL] != ev[3])
                    seen["restored_end"] += bool(cur[ref.BITS] & ref.FROM_RESTORE)
            elif ev[0] in (ref.EV_RESET, ref.EV_RESTORE):
                seen["reset_empty" if cur[ref.STEPS] == 0 else "reset_running"] += 1
                seen["restore"] += ev[0] == ref.EV_RESTORE
            elif ev[0] == ref.EV_TICK:
                seen["tick"] += 1
            else:
                seen["clear"] += 1
            before = sum(t[ref.COL["abandoned"]] for t in table)
            end = ref.apply_events(model, table, auto, [ev], [r])
            seen["abandoned"] += sum(t[ref.COL["abandoned"]] for t in table) - before
            any_end |= end
            i, d, t, e = _apply_native(lib, native, ntable, auto, [ev], [r])
            native.i, native.d, ntable = [int(v) for v in i], [float(v) for v in d], [[int(v) for v in q] for q in t]
            assert e == int(end) and _same(model, table, i, d, t), (seed, ev, list(i), model.i)
        i, d, t, e = _apply_native(lib, ref.Record(), ref.new_table(n_levels), auto, events, rows)   # and the whole list in one call
        assert e == int(any_end) and _same(model, table, i, d, t), seed
        assert all(row[13:] == [0, 0, 0] for row in table)
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("ret, want", [
    (0.0, 0), (1.0, 1 << 20), (-1.0, -(1 << 20)),
    (2.5 * 2.0 ** -20, 3), (3.5 * 2.0 ** -20, 4), (-2.5 * 2.0 ** -20, -2), (-3.5 * 2.0 ** -20, -3),   # ties go up: floor(v + 0.5)
    (np.nextafter(2.5 * 2.0 ** -20, 0.0), 2), (np.nextafter(-2.5 * 2.0 ** -20, -1.0), -3),                # one ulp off the tie
    (0.49999 * 2.0 ** -20, 0), (-0.49999 * 2.0 ** -20, 0), (-0.5 * 2.0 ** -20, 0), (-0.50001 * 2.0 ** -20, -1),
    (-123.456, None), (2.0 ** 42, 1 << 62), (2.0 ** 43, 1 << 62), (float("inf"), 1 << 62), (-2.0 ** 42, -(1 << 62)), (-1e300, -(1 << 62)),
    (float("-inf"), -(1 << 62)), (float("nan"), 0), (2.0 ** 42 - 2.0 ** -11, (1 << 62) - 512),
])
def test_return_fix_column(ret, want):
    """the table's return column of one episode whose return is `ret`: the model and the host entry, against the written value"""
    from nclone_amd import _native as nat

    ret = float(ret)
    if want is None:
        import math
        want = math.floor(ret * 2 ** 20 + 0.5)
    assert ref.return_fix(ret) == want & ref.M64
    rec = ref.Record()
    rec.d[ref.RET] = ret
    rec.i[ref.STEPS] = 3   # (a running episode: the row below does not take a new level)
    rec.i[ref.LEVEL] = 0
    ev = np.array([[ref.EV_ROW, ref.F_DEAD, 1, 0, 0, 0, 0, 0]], dtype=np.int32)
    i, d, t, e = _apply_native(nat.lib(), rec, ref.new_table(1), True, ev, np.zeros((1, 8), dtype=np.float32))
    assert e == 1 and int(t[0, ref.COL["return_fix"]]) == want & ref.M64 and int(t[0, ref.COL["episodes"]]) == 1
    if ret == ret:
        assert d[ref.DFIN + ref.RET] == ret and d[ref.RET] == 0.0
        assert abs(ref.fix_to_float(t[0, ref.COL["return_fix"]]) - min(max(ret, -2.0 ** 42), 2.0 ** 42)) <= 2.0 ** -21


def test_negative_and_positive_returns_cancel_in_the_table():
    from nclone_amd import _native as nat

    table = ref.new_table(1)
    rec = ref.Record()
    ev = np.array([[ref.EV_ROW, ref.F_DEAD, 4, 0, 0, 0, 0, 0], [ref.EV_ROW, ref.F_WON, 4, 0, 0, 0, 0, 0]], dtype=np.int32)
    rows = np.zeros((2, 8), dtype=np.float32)
    rows[0, 0], rows[1, 0] = -7.25, 7.25
    i, d, t, e = _apply_native(nat.lib(), rec, table, True, ev, rows)
    assert int(t[0, ref.COL["return_fix"]]) == 0 and int(t[0, ref.COL["episodes"]]) == 2 and int(t[0, ref.COL["won_frames"]]) == 4


def test_host_entry_under_asan_and_ubsan(tmp_path):
    """npp_episode_apply_host in a stand-alone program (tests/episode_sanitized_main.cpp) built with g++ -fsanitize=address,undefined
    together with the host sources, runtimes linked statically: on seeded lists it must print the model's record and table, apply
    event by event to the same end, pass its zero-length / largest-level cases and refuse its bad arguments, with no sanitizer report."""
    from nclone_amd import build_native

    exe = str(tmp_path / "episode_sanitized_main")
    srcs = [os.path.join(build_native.CSRC, f) for f in build_native.HOST_SOURCES]
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-static-libasan",
                        "-static-libubsan", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "episode_sanitized_main.cpp")] + srcs + ["-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=23", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for seed, n_levels, auto, comps in ((1, 1, 1, True), (2, 3, 0, False), (3, 4, 1, False)):
        rng = np.random.default_rng(100 + seed)
        events, rows = ref.random_events(rng, n_levels, 300, comps)
        events.tofile(str(tmp_path / "events.bin"))
        rows.tofile(str(tmp_path / "rows.bin"))
        r = subprocess.run([exe, str(tmp_path / "events.bin"), str(tmp_path / "rows.bin"), str(len(events)), str(n_levels), str(auto)],
                           capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, (seed, r.returncode, r.stdout[-500:], r.stderr[-3000:])
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
        out = r.stdout.split("\n")
        model, table = ref.Record(), ref.new_table(n_levels)
        end = ref.apply_events(model, table, bool(auto), events, rows)
        assert out[0] == "applied 0 %d 1" % int(end), out[0]
        assert [int(v) for v in out[1].split()] == model.i
        assert [float.fromhex(v) for v in out[2].split()] == model.d
        assert [int(v) for v in out[3].split()] == [v for row in table for v in row]
        assert out[4] == "edge ok 14 refused 11", out[4]


def test_argument_checks_need_no_device():
    from nclone_amd.async_env import NppAsyncVecEnvironment
    from nclone_amd.engine import NppBatch
    from nclone_amd.vec_env import NppVecEnvironment

    with pytest.raises(ValueError, match="episode_stats"):
        NppAsyncVecEnvironment([np.zeros(1)], 64, episode_stats=True)
    v = object.__new__(NppVecEnvironment)
    v._episode = False
    for call in (v.episode_level_stats, v.reset_episode_level_stats):
        with pytest.raises(RuntimeError, match="created without episode_stats"):
            call()
    b = object.__new__(NppBatch)
    b.n = 4
    b.flags, b.frames, b.reward = torch.zeros(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.int16), torch.zeros(4)
    with pytest.raises(ValueError, match="episode_accumulate: flags must be a contiguous uint8 CUDA tensor"):
        b.episode_accumulate()
    with pytest.raises(ValueError, match="episode_restart: mask must be"):
        b.episode_restart(torch.zeros(4, dtype=torch.uint8))
    assert NppBatch.EPISODE_COLUMNS == ref.COLUMNS
    b.h = None   # (nothing to destroy)
