"""CPU checks of seeding the cell index from replays (include/npp_amd.h npp_archive_seed): the per-tick rows of the
rule (npp_archive_seed_rows_host) against the reference's two byte functions on all 256 byte values and against the seeder's
progress score; the conditions tests/golden/seed.npz was chosen for; the citations of the header and of DESIGN.md; the expected
table the restatement (tests/seed_ref.py) builds from the reference's checkpoints, which tests/test_gpu_seed.py compares the device
with."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tests import cell_archive_ref as cref
from tests import seed_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"npp_archive_seed": 8, "npp_archive_seed_rows_host": 6}


@pytest.fixture(scope="module")
def nat():
    from nclone_amd import build_native

    build_native.build()
    from nclone_amd import _native

    return _native


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _rows(nat, inputs, mode):
    inp = np.ascontiguousarray(inputs, dtype=np.uint8)
    n = len(inp)
    actions, bits = np.full(n, 99, dtype=np.uint8), np.full(n, 99, dtype=np.uint8)
    scores = np.full(n, -7.0, dtype=np.float32)
    rc = nat.lib().npp_archive_seed_rows_host(_p(inp), n, mode, _p(actions), _p(bits), _p(scores))
    return rc, actions, bits, scores


def _reference_byte_functions():
    """map_input_to_action / decode_input_to_controls as the reference's own functions answered for every byte value
    (replay/replay_executor.py:42-84; recorded by make_golden_seed.py), and the controls each action presses."""
    z = sref.fixture()
    controls_of_action = {0: (0, 0), 1: (-1, 0), 2: (1, 0), 3: (0, 1), 4: (-1, 1), 5: (1, 1)}
    return (lambda b: int(z["byte_action"][b])), (lambda b: tuple(int(v) for v in z["byte_controls"][b])), controls_of_action


def test_entries_declared_exported_and_bound(nat):
    hdr = open(os.path.join(ROOT, "include", "npp_amd.h")).read()
    lib = nat.lib()
    for name, argc in ENTRIES.items():
        assert "int %s(" % name in hdr, name
        assert name in nat.EXPORTS, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == argc and fn.restype is C.c_int, name
    assert lib.npp_archive_seed(None, None, None, None, 0, 0, None, None) == nat.NPP_ERR_INVALID
    assert lib.npp_archive_seed_rows_host(None, 3, 0, None, None, None) == nat.NPP_ERR_INVALID
    assert lib.npp_archive_seed_rows_host(None, -1, 0, None, None, None) == nat.NPP_ERR_INVALID
    one = np.zeros(1, dtype=np.uint8)
    for mode in (2, 3, -1):   # the table mode has no host rows
        assert lib.npp_archive_seed_rows_host(_p(one), 1, mode, None, None, None) == nat.NPP_ERR_INVALID
    assert lib.npp_archive_seed_rows_host(None, 0, 0, None, None, None) == nat.NPP_OK


def test_header_and_design_citations():
    hdr = open(os.path.join(ROOT, "include", "npp_amd.h")).read()
    block = hdr[hdr.index("Seeding the cell index from recorded replays"):hdr.index("int npp_archive_seed_rows_host(")]
    for cite in ("demo_checkpoint_seeder.py", ":667-809", ":777-779", ":118-153", ":310-312", "npp_demo_plan_host", "deviation",
                 "72 px", "neither visits nor chosen", "b == 7", "{0, 6}", "complete or not at all"):
        assert cite in block, cite
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"^## 22\. .*$", design, flags=re.M)
    assert m, "DESIGN.md has no section 22"
    sec = design[m.start():]
    for cite in ("demo_checkpoint_seeder.py", ":777-779", "pbrs_potentials.py:158", ":69-116", ":310-312", "npp_archive_seed", "no_count",
                 "Launches per tick"):
        assert cite in sec, cite


def test_rows_host_on_all_256_bytes(nat):
    """Actions and the mismatch latch against the reference's two functions, every byte value on its own and in sequences."""
    to_action, decode, controls = _reference_byte_functions()
    mismatch = [controls[to_action(b)] != decode(b) for b in range(256)]
    assert [b for b in range(256) if mismatch[b]][:6] == [7, 9, 10, 11, 12, 13] and not mismatch[6] and not mismatch[8] and not mismatch[14]
    assert mismatch == [sref.byte_mismatch(b) for b in range(256)]
    for b in range(256):   # one byte behind three clean ones: the latch starts exactly at it
        rc, actions, bits, _ = _rows(nat, [0, 2, 5, b, 1, 0], 0)
        assert rc == 0
        assert actions.tolist() == [0, 2, 4, to_action(b), 3, 0], b
        assert bits.tolist() == [0, 0, 0] + [2 if mismatch[b] else 0] * 3, b
    rng = np.random.default_rng(3)
    for _ in range(50):
        seq = rng.integers(0, 256, size=int(rng.integers(1, 300))).astype(np.uint8)
        if rng.random() < 0.5:
            seq = seq & 7   # recorder bytes only
        rc, actions, bits, _ = _rows(nat, seq, 1)
        assert rc == 0
        assert actions.tolist() == [to_action(int(b)) for b in seq]
        first = next((k for k, b in enumerate(seq) if mismatch[int(b)]), len(seq))
        assert bits.tolist() == [0] * first + [2] * (len(seq) - first)
        assert np.array_equal(actions, sref.route_of(seq, len(seq) - 1))


def test_rows_host_scores(nat):
    for L in (1, 2, 3, 7, 19, 21, 22, 121, 1000, 65534):
        seq = np.zeros(L, dtype=np.uint8)
        rc, _, _, s = _rows(nat, seq, 0)
        want = np.array([f / max(1, L) for f in range(L)], dtype=np.float64).astype(np.float32)   # frame_idx / max(1, total_frames)
        assert rc == 0 and np.array_equal(s.view(np.uint32), want.view(np.uint32)), L
        rc, _, _, s = _rows(nat, seq, 1)
        want = (-(np.arange(L) + 1).astype(np.float32)).astype(np.float32)
        assert rc == 0 and np.array_equal(s.view(np.uint32), want.view(np.uint32)), L
    z = sref.fixture()
    for r in range(len(z["src"])):   # the reference's own cumulative_reward of every returned checkpoint
        sel = z["cp_replay"] == r
        if not sel.any():
            continue
        rc, _, _, s = _rows(nat, z["in%d" % r], 0)
        assert np.array_equal(s[z["cp_frame"][sel]].view(np.uint32), z["cp_reward"][sel].astype(np.float32).view(np.uint32)), r


def test_fixture_conditions():
    z = sref.fixture()
    assert bytes(z["mode"]).decode() == "seeder"   # DemoCheckpointSeeder._extract_positions_from_demo_simple itself produced the rows
    R = len(z["src"])
    assert R == 8 and z["success"].tolist() == [1] * 7 + [0]
    maps = [bytes(z["m%d" % r]) for r in range(R)]
    assert maps[0] != maps[1] and maps[2] not in maps[:2] and maps[3] == maps[0] and maps[4] == maps[0] and maps[5] == maps[1]
    assert maps[6] not in maps[:3]
    assert np.array_equal(z["in3"], z["in0"]) and np.array_equal(z["in4"], z["in0"][:len(z["in4"])]) and len(z["in4"]) < len(z["in0"])
    t7 = int(z["byte7_tick"][0])
    assert z["in5"][t7] == 7 and np.array_equal(np.delete(z["in5"], t7), np.delete(z["in1"], t7)) and 7 not in z["in1"]
    assert all(len(z["in%d" % r]) == z["L"][r] for r in range(R)) and z["L"].max() < 200
    assert np.array_equal(z["cp_seq_len"], z["cp_frame"] + 1)   # FULL action sequence from the spawn
    assert np.array_equal(z["cp_action"], [sref.ACTION_OF_BYTE[z["in%d" % r][f]] if z["in%d" % r][f] < 8 else 0
                                           for r, f in zip(z["cp_replay"], z["cp_frame"])])
    # the prefix ends before the first replay's switch
    on0 = z["cp_frame"][(z["cp_replay"] == 0) & (z["cp_switch"] != 0)]
    kept0 = set(z["cp_frame"][z["cp_replay"] == 0].tolist())
    first_on = min([int(f) for f in on0] + [f for f in range(int(z["L"][0])) if f not in kept0])
    assert len(z["in4"]) <= first_on and not z["cp_switch"][z["cp_replay"] == 4].any()
    # (1) a checkpoint with the switch on; (2) a tick dropped by the 72 px filter
    assert int(z["cp_switch"].sum()) >= 1
    dropped = sum(int(z["break_tick"][r]) + 1 - int((z["cp_replay"] == r).sum()) for r in range(R) if z["break_tick"][r] >= 0)
    assert dropped >= 1
    # (3) a cell a later replay wins over an earlier one, in the caller's order
    best = {}
    for r, f, p, sw, rew in zip(z["cp_replay"], z["cp_frame"], z["cp_pos"], z["cp_switch"], z["cp_reward"]):
        d = best.setdefault((maps[r], int(sw), math.floor(p[0] / 24.0), math.floor(p[1] / 24.0)), {})
        d[int(r)] = max(d.get(int(r), -1.0), float(rew))
    later = [k for k, d in best.items() if len(d) > 1 and max(d, key=lambda r: (d[r], -r)) > min(d) and d[max(d, key=lambda r: (d[r], -r))] > d[min(d)]]
    assert len(later) >= 1
    # (4) no position within 1e-3 px of a cell border or of the 72 px circle: a last-bit difference cannot move a key
    for r, p in zip(z["cp_replay"], z["cp_pos"]):
        for v in p:
            assert abs(v / 24.0 - round(v / 24.0)) * 24.0 >= 1e-3, (r, p)
        assert abs(math.hypot(p[0] - z["door"][r][0], p[1] - z["door"][r][1]) - 72.0) >= 1e-3, (r, p)
    # the reference appended no death tick here (every played replay ends won or alive), so the deviation costs no checkpoint
    assert all(int(s) in (0, 1, 2, 3, 4, 5, 8, -1) for s in z["end_state"])


@pytest.mark.parametrize("n_envs", [1, 3, 8])
def test_expected_table(nat, n_envs):
    """The restatement on the fixture: statuses, the tie rule, cross-replay competition, the exit filter and the full archive."""
    z = sref.fixture()
    reps = sref.Replays(z)
    assert reps.status.tolist() == [0, 0, 0, 0, 0, 0, 1, 2] and reps.played == [0, 1, 2, 3, 4, 5] and len(reps.levels) == 3
    X = sref.Expected(reps, n_envs, 64)
    assert 0 < X.n_used <= 64 and X.overflow == 0
    assert X.counts[:, 0].tolist() == [21, 22, 121, 21, 19, 22, 0, 0]
    assert X.counts[:, 1].tolist() == [int((z["cp_replay"] == r).sum()) for r in range(6)] + [0, 0]
    assert (X.cell_slot >= 0).sum() == X.n_used and sorted(X.slot_key[:X.n_used].tolist()) == sorted(np.flatnonzero(X.cell_slot >= 0).tolist())
    # every slot holds the best score of its cell over all played replays; the identical copy (replay 3) never displaces replay 0
    # from a cell both reach at the same tick -- the incumbent, or inside one tick the lower env, wins the tie
    best = {}
    for r in reps.played:
        for f, (k, _, _) in reps.ticks[r].items():
            best[k] = max(best.get(k, 0), cref.ordered_bits(sref.score_of("progress", r, f, len(reps.inputs[r]))))
    for k, ob in best.items():
        assert cref.ordered_bits(X.cell_score[k]) == ob
    srcs = [r for r, _ in X.slot_src.values()]
    stored = {r for r, _, _, _ in X.events}   # (the schedule, longest first and ties by index, puts replay 0 before its copy for every n_envs)
    assert 0 in stored and 3 not in stored and X.counts[0, 2] >= 1 and X.counts[3, 2] == 0 and X.counts[3, 1] == X.counts[0, 1]
    assert 4 in srcs   # the prefix scores f / 19 > f / 21 on the same states: a later replay (caller's order) takes cells of replay 0
    assert any(old >= 0 and old != r for r, _, _, old in X.events)   # a stored record was replaced by another replay's
    assert any(reps.ticks[r][f][2] for r, f in X.slot_src.values())  # a cell behind the switch
    # 8 slots: the first 8 new cells in call order hold them, the rest overflow
    F = sref.Expected(reps, n_envs, 8)
    assert F.n_used == 8 and F.overflow > 0 and F.slot_key.tolist() == [k for k in F.slot_key if k >= 0]
    firsts = []
    for r, f, slot, old in X.events:
        if old < 0 and len(firsts) < 8:
            firsts.append(int(X.slot_key[slot]))
    assert F.slot_key.tolist() == firsts


def test_rows_under_asan_and_ubsan(nat, tmp_path):
    """npp_archive_seed_rows_host in a stand-alone program (tests/seed_sanitized_main.cpp) built with g++
    -fsanitize=address,undefined together with the host sources, runtimes linked statically: random byte sequences (length 0
    included), both modes and a refused mode must give the library's rows and no sanitizer report."""
    import struct
    import subprocess

    from nclone_amd import build_native

    exe = str(tmp_path / "seed_sanitized_main")
    srcs = [os.path.join(build_native.CSRC, f) for f in build_native.HOST_SOURCES]
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-static-libasan",
                        "-static-libubsan", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "seed_sanitized_main.cpp")] + srcs + ["-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    rng = np.random.default_rng(8)
    sets = [(rng.integers(0, 256, size=int(n)).astype(np.uint8), int(mode)) for n, mode in
            [(0, 0), (1, 1), (7, 0), (300, 1), (64, 0), (5, 2), (2000, 0)] + [(rng.integers(1, 200), rng.integers(0, 2)) for _ in range(30)]]
    path = str(tmp_path / "sets.bin")
    with open(path, "wb") as f:
        for seq, mode in sets:
            f.write(struct.pack("<Ib", len(seq), mode) + seq.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=23", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.split("\n")
    assert len(lines) >= 4 * len(sets)
    for k, (seq, mode) in enumerate(sets):
        got = [[int(x) for x in lines[4 * k + i].split()] for i in range(4)]
        rc, actions, bits, scores = _rows(nat, seq, mode)
        assert got[0] == [rc]
        if mode == 2:   # refused: NPP_ERR_INVALID and nothing written
            assert rc == 1 and got[1] == [99] * len(seq) and got[2] == [99] * len(seq)
            continue
        assert rc == 0 and got[1] == actions.tolist() and got[2] == bits.tolist() and got[3] == scores.view(np.uint32).tolist()
