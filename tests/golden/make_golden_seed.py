#!/usr/bin/env python3
"""Golden checkpoints for seeding the cell index from replays, produced by RUNNING the reference's
DemoCheckpointSeeder._extract_positions_from_demo_simple (nclone/replay/demo_checkpoint_seeder.py:667-809) on replays of
corpus.npz (build container only; data only, byte-reproducible).

    HOME=/tmp/orahome PYTHONPATH=/root/reference python3 tests/golden/make_golden_seed.py      # -> seed.npz

Every replay is written to a scratch .replay file (the recorder's V1 format) and handed to the seeder's own method; what it
returns is recorded as it is.  The stand-ins that let the reference import are make_golden_demo._stand_ins().  When the seeder
cannot be constructed, the second way ("loop": the executor's two byte functions from its file and NPlayHeadless driven in the
seeder's loop, with its filter and its break) is taken, in the manner of make_golden_demo; `mode` says which way produced the file.

Replays (corpus.npz indices are chosen by the search below, the shortest that do the job; `src` records them):
  0  a very_simple win                       1  a very_simple win on another map          2  a win on a map with toggle mines
  3  an identical copy of 0 (equal scores: the tie rule)
  4  a prefix of 0 cut before its switch (same frames, another L: cross-replay competition on one level)
  5  a copy of 1 with one mid-air byte replaced by 7 (route bit 2)
  6  a win on a map no test env loads        7  a copy of another win with success byte 0 (skipped by the env method; not played)

Output seed.npz:
  mode      bytes "seeder" or "loop"
  src       i32[R] corpus index; success u8[R]; L i32[R]; break_tick i32[R] (the tick at which the reference's loop broke, L - 1 when
            it ran out of inputs, -1 for the replay that is not played); end_state i32[R] (the ninja's state after that tick: 8 won, 6 / 7
            dead -- a checkpoint AT the break tick of a death is the reference's, not the index's); byte7_tick i32[1] (the tick of replay 5 that holds byte 7)
  m<r> in<r>         map bytes / input bytes as played
  per returned checkpoint, in the order returned, replay after replay:
    cp_replay i32, cp_frame i32 (frame_idx), cp_pos f64[., 2], cp_switch u8 (switch_activated), cp_reward f64 (cumulative_reward),
    cp_action u8, cp_seq_len i32 (len(action_sequence))
  byte_action u8[256], byte_controls i8[256, 2]   map_input_to_action(b) and decode_input_to_controls(b) = (horizontal, jump) of the
                     reference (replay/replay_executor.py:42-84) for every byte value
  door f64[R, 2]     exit_door_position() of the replay's level (what the seeder's filter measures against)
"""
import math
import os
import struct
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_demo as mgd  # noqa: E402

EPS = 1e-3


def replay_bytes(m, inp, success=True):
    return struct.pack("<III", 1, len(m), len(inp)) + struct.pack("<B", 1 if success else 0) + bytes(m) + bytes(inp)


def make_runner():
    """-> (mode, run(map_bytes, inputs) -> (checkpoint dicts, break tick, door position, ninja state after the last tick))"""
    mgd._stand_ins()
    import nclone.nplay_headless as nph

    calls = {"n": 0, "door": None, "state": -1}
    inner_tick = nph.NPlayHeadless.tick

    def counting_tick(self, *a, **k):
        calls["n"] += 1
        r = inner_tick(self, *a, **k)
        calls["door"] = tuple(float(v) for v in self.exit_door_position())
        calls["state"] = int(self.sim.ninja.state)
        return r

    nph.NPlayHeadless.tick = counting_tick
    try:
        from nclone.replay.demo_checkpoint_seeder import DemoCheckpointSeeder

        seeder = DemoCheckpointSeeder(replay_dir=tempfile.gettempdir())

        def run(m, inp):
            with tempfile.TemporaryDirectory() as d:
                p = os.path.join(d, "20250101_000000_seed.replay")
                with open(p, "wb") as f:
                    f.write(replay_bytes(m, inp))
                calls["n"] = 0
                from pathlib import Path

                cps = seeder._extract_positions_from_demo_simple(Path(p))
            assert calls["n"] >= 1, "the seeder played nothing (its except branch swallowed an error)"
            return cps, calls["n"] - 1, calls["door"], calls["state"]

        c = np.load(os.path.join(HERE, "corpus.npz"))
        run(c["m3"], c["in3"][:2])
        return "seeder", run
    except Exception as e:   # noqa: BLE001 -- any failure to import or construct: the documented second way
        import traceback

        print("DemoCheckpointSeeder unavailable (%s: %s): driving NPlayHeadless in its loop\n%s"
              % (type(e).__name__, e, "".join(traceback.format_tb(e.__traceback__)[-3:])), flush=True)
    decode, to_action = mgd._executor_file_functions()

    def run(m, inp):
        hp = nph.NPlayHeadless(render_mode="grayscale_array", enable_animation=False, enable_logging=False, enable_debug_overlay=False,
                               seed=42, enable_rendering=False)
        hp.load_map_from_map_data(list(bytes(m)))
        seq, cps, actions = [int(b) for b in inp], [], []
        calls["n"] = 0
        for frame_idx, b in enumerate(seq):
            h, j = decode(b)
            actions.append(to_action(b))
            hp.tick(h, j)
            x, y = hp.ninja_position()
            pos = (float(x), float(y))
            sw = hp.exit_switch_activated()
            door = hp.exit_door_position()
            near = sw and ((pos[0] - door[0]) ** 2 + (pos[1] - door[1]) ** 2) ** 0.5 < 72.0
            if not near:
                cps.append({"cumulative_reward": frame_idx / max(1, len(seq)), "action": actions[-1], "frame_idx": frame_idx,
                            "switch_activated": sw, "position": pos, "action_sequence": list(actions)})
            if hp.ninja_has_won() or hp.sim.ninja.has_died():
                break
        return cps, calls["n"] - 1, calls["door"], calls["state"]

    return "loop", run


def clear_of_borders(cps, door):
    """No recorded position within EPS of a 24 px cell border or of the 72 px circle around the door."""
    for cp in cps:
        x, y = cp["position"]
        for v in (x, y):
            q = v / 24.0
            if abs(q - round(q)) * 24.0 < EPS:
                return False
        if abs(math.hypot(x - door[0], y - door[1]) - 72.0) < EPS:
            return False
    return True


def cell_of(cp):
    return (int(bool(cp["switch_activated"])), math.floor(cp["position"][0] / 24.0), math.floor(cp["position"][1] / 24.0))


def main():
    c = np.load(os.path.join(HERE, "corpus.npz"))
    names = bytes(c["names"]).decode().split("\n")
    sigs = bytes(c["sigs"]).decode().split("\n")
    mode, run = make_runner()
    print("mode:", mode, flush=True)
    by_len = sorted(range(len(names)), key=lambda i: (len(c["in%d" % i]), i))
    played = {}

    def play(i, inp=None):
        key = (i, None if inp is None else bytes(inp))
        if key not in played:
            played[key] = run(c["m%d" % i], c["in%d" % i] if inp is None else inp)
        return played[key]

    def good(i, inp=None, need_win=True):
        cps, brk, door, _ = play(i, inp)
        L = len(c["in%d" % i] if inp is None else inp)
        won = brk < L - 1 or not cps or cps[-1]["frame_idx"] != L - 1   # the loop broke, or the last tick was filtered at the door
        return clear_of_borders(cps, door) and (won or not need_win) and len(cps) > 0

    simple = [i for i in by_len if "very_simple" in names[i]]
    mined = [i for i in by_len if "1" in sigs[i].split(",")]
    r0 = next(i for i in simple if good(i))
    r1 = next(i for i in simple if bytes(c["m%d" % i]) != bytes(c["m%d" % r0]) and good(i))
    r2 = next(i for i in mined if good(i) and any(cp["switch_activated"] for cp in play(i)[0]))   # (far from the door with the switch on)
    used_maps = {bytes(c["m%d" % i]) for i in (r0, r1, r2)}
    r6 = next(i for i in simple if bytes(c["m%d" % i]) not in used_maps and good(i))
    r7 = next(i for i in simple if i not in (r0, r1, r6))
    in0, in1 = np.array(c["in%d" % r0], dtype=np.uint8), np.array(c["in%d" % r1], dtype=np.uint8)
    kept = {cp["frame_idx"]: cp["switch_activated"] for cp in play(r0)[0]}   # a tick the filter dropped had the switch on
    first_on = min(f for f in range(len(in0)) if kept.get(f, True))
    cut = next(k for k in range(first_on, 1, -1) if good(r0, in0[:k], need_win=False))   # the prefix ends before the switch
    byte7 = None
    for t in sorted(range(2, len(in1) - 2), key=lambda t: abs(t - len(in1) // 2)):   # from the middle outwards
        trial = in1.copy()
        trial[t] = 7
        if good(r1, trial, need_win=False) and len(play(r1, trial)[0]) > t + 2:
            byte7, in5 = t, trial
            break
    assert byte7 is not None
    src = [r0, r1, r2, r0, r0, r1, r6, r7]
    inputs = [in0, in1, np.array(c["in%d" % r2], dtype=np.uint8), in0.copy(), in0[:cut].copy(), in5,
              np.array(c["in%d" % r6], dtype=np.uint8), np.array(c["in%d" % r7], dtype=np.uint8)]
    success = np.array([1, 1, 1, 1, 1, 1, 1, 0], dtype=np.uint8)
    out = {"mode": np.frombuffer(mode.encode(), dtype=np.uint8), "src": np.array(src, dtype=np.int32), "success": success,
           "L": np.array([len(x) for x in inputs], dtype=np.int32), "byte7_tick": np.array([byte7], dtype=np.int32)}
    cols = {k: [] for k in ("replay", "frame", "pos", "switch", "reward", "action", "seq_len")}
    brk, doors, per, ends = [], [], [], []
    for r, (i, inp) in enumerate(zip(src, inputs)):
        out["m%d" % r], out["in%d" % r] = np.array(c["m%d" % i], dtype=np.uint8), inp
        if not success[r]:
            brk.append(-1)
            ends.append(-1)
            doors.append((0.0, 0.0))
            per.append([])
            continue
        cps, b, door, end = run(out["m%d" % r], inp)
        brk.append(b)
        ends.append(end)
        doors.append(door)
        per.append(cps)
        assert clear_of_borders(cps, door), r
        for cp in cps:
            assert list(cp["action_sequence"][-1:]) == [cp["action"]]
            cols["replay"].append(r); cols["frame"].append(cp["frame_idx"]); cols["pos"].append(cp["position"])
            cols["switch"].append(1 if cp["switch_activated"] else 0); cols["reward"].append(cp["cumulative_reward"])
            cols["action"].append(cp["action"]); cols["seq_len"].append(len(cp["action_sequence"]))
    decode, to_action = mgd._executor_file_functions()   # the reference's two byte functions on every byte value
    out["byte_action"] = np.array([to_action(b) for b in range(256)], dtype=np.uint8)
    out["byte_controls"] = np.array([decode(b) for b in range(256)], dtype=np.int8)
    out["break_tick"] = np.array(brk, dtype=np.int32)
    out["end_state"] = np.array(ends, dtype=np.int32)
    out["door"] = np.array(doors, dtype=np.float64)
    out["cp_replay"] = np.array(cols["replay"], dtype=np.int32)
    out["cp_frame"] = np.array(cols["frame"], dtype=np.int32)
    out["cp_pos"] = np.array(cols["pos"], dtype=np.float64).reshape(-1, 2)
    out["cp_switch"] = np.array(cols["switch"], dtype=np.uint8)
    out["cp_reward"] = np.array(cols["reward"], dtype=np.float64)
    out["cp_action"] = np.array(cols["action"], dtype=np.uint8)
    out["cp_seq_len"] = np.array(cols["seq_len"], dtype=np.int32)
    # the conditions the tests assert again from the file
    switched = int(out["cp_switch"].sum())
    dropped = sum(int(b) + 1 - len(cps) for b, cps in zip(brk, per) if b >= 0)
    best = {}   # (level map, cell) -> list of (replay, best score there)
    for r, cps in enumerate(per):
        for cp in cps:
            k = (bytes(out["m%d" % r]),) + cell_of(cp)
            d = best.setdefault(k, {})
            d[r] = max(d.get(r, -1.0), cp["cumulative_reward"])
    later_wins = sum(1 for d in best.values() if len(d) > 1 and max(d, key=lambda r: (d[r], -r)) > min(d) and
                     d[max(d, key=lambda r: (d[r], -r))] > d[min(d)])
    print("replays", src, "L", out["L"].tolist(), "break", brk, "cut", cut, "byte 7 at tick", byte7)
    print("checkpoints %d, with the switch on %d, ticks dropped by the 72 px filter %d, cells a later replay wins %d"
          % (len(out["cp_frame"]), switched, dropped, later_wins))
    assert switched >= 1 and dropped >= 1 and later_wins >= 1
    p = os.path.join(HERE, "seed.npz")
    mgd._save_reproducible(p, out)
    print("seed.npz", os.path.getsize(p), "bytes")
    assert os.path.getsize(p) < 300 * 1024


if __name__ == "__main__":
    main()
