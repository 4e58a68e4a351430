#!/usr/bin/env python3
"""Golden demonstration transitions, produced by RUNNING the reference's ReplayExecutor.execute_replay
(nclone/replay/replay_executor.py:304-462) on replays of corpus.npz (build container only; data only, byte-reproducible).

    HOME=/tmp/orahome PYTHONPATH=/root/reference python3 tests/golden/make_golden_demo.py      # -> demo.npz

How the reference is run: nclone.replay imports observation_processor.py, which imports cv2 (absent in the build container), and
the package __init__ of nclone.gym_environment needs gymnasium.  An empty stand-in `cv2` module is put into sys.modules (the
executor runs with enable_rendering=False and the processor with enable_visual_processing=False, so no cv2 function is ever
called), a permissive stand-in `gymnasium` in the manner of make_golden_stack.py (the env classes that name its spaces are defined,
never instantiated), and the two generated tables the executor's GraphBuilder loads are made by the reference's own precomputers
on a scratch copy of the package (make_golden_reach.prepare()).  With them
    ReplayExecutor(enable_rendering=False, frame_skip=fs).execute_replay(map_data, inputs)
ITSELF runs, and THAT IS WHAT HAPPENED for the committed demo.npz: its `mode` member says "executor".  The second way, "loop" (the
executor's decode_input_to_controls / map_input_to_action loaded from its file and NPlayHeadless driven in the executor's loop with
its time_remaining lines), is taken only when the executor cannot be constructed; run once for comparison it gave the same bytes
in every array.  The rows are what the executor's own _get_raw_observation returned at every sampled frame (captured by wrapping the
bound method; nothing is recomputed here).

Replays (corpus.npz indices): 3, 60, 58, 0, 74, 127 (a door level), 13 (28 entities) as recorded, and index 0 truncated to 3
ticks (L < fs for fs = 4).  When no chosen replay's inputs continue past its win, 8 NOOP bytes are appended to replay 3's inputs
(r0 below then differs from corpus in3 by those bytes; `padded` says so).

Output demo.npz:
  mode      bytes "executor" or "loop"
  src       i32[R]   corpus index of replay r;  padded u8[R]: NOOP bytes appended;  fs i32[2] = 1, 4
  m<r> in<r>         map bytes / input bytes as played
  per frame skip s in (1, 4):
    s<s>_frame<r> i32[rows], s<s>_action<r> u8[rows], s<s>_gs<r> f32[rows, 41] (game_state as the executor builds it),
    s<s>_pos<r> f64[rows, 6] (player, switch, exit door), s<s>_flags<r> u8[rows] (1 won | 2 dead | 4 switch activated)
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
if REF not in sys.path:
    sys.path.insert(0, REF)

SRC = [3, 60, 58, 0, 74, 127, 13, 0]
CUT = {7: 3}          # entry 7: replay 0 truncated to 3 ticks
FRAME_SKIPS = (1, 4)
PAD = 8


def _stand_ins():
    # the executor's GraphBuilder reads two generated tables the reference does not ship: make_golden_reach.prepare() copies the
    # package to a scratch directory, runs the reference's own precomputers there and registers nclone.gym_environment as a bare
    # package (its __init__ needs gymnasium)
    sys.path.insert(0, HERE)
    import make_golden_reach

    make_golden_reach.prepare()
    global REF
    REF = make_golden_reach.REF
    for n in [n for n in sys.modules if n.startswith("nclone")]:   # with the gymnasium stand-in below the real package __init__s run
        del sys.modules[n]
    if "cv2" not in sys.modules:
        try:
            import cv2  # noqa: F401
        except ImportError:
            sys.modules["cv2"] = types.ModuleType("cv2")
    try:
        import gymnasium  # noqa: F401
    except ImportError:
        class Anything:
            def __init__(self, *a, **k):
                pass

        class Permissive(types.ModuleType):
            """any name imported from it is an empty class or (lower case) the module itself: the env classes that name them
            are defined but never instantiated here"""
            __path__ = []

            def __getattr__(self, name):
                if name.startswith("__"):
                    raise AttributeError(name)
                v = self if name[0].islower() else type(name, (Anything,), {})
                setattr(self, name, v)
                return v

        gym = Permissive("gymnasium")
        for n in ("gymnasium", "gymnasium.spaces", "gymnasium.spaces.box", "gymnasium.spaces.discrete", "gymnasium.utils",
                  "gymnasium.envs", "gymnasium.envs.registration", "gymnasium.wrappers"):
            sys.modules[n] = gym


def _executor_file_functions():
    """decode_input_to_controls / map_input_to_action of replay_executor.py without importing the package around it: only the
    two module-level functions are compiled, from the file's own text."""
    import ast

    path = os.path.join(REF, "nclone", "replay", "replay_executor.py")
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("decode_input_to_controls", "map_input_to_action")]
    ns = {}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns["decode_input_to_controls"], ns["map_input_to_action"]


def make_runner():
    """-> (mode, run(map_bytes, inputs, fs) -> list of (frame, action, raw observation dict))"""
    _stand_ins()
    try:
        from nclone.replay.replay_executor import ReplayExecutor

        def run(m, inp, fs):
            ex = ReplayExecutor(enable_rendering=False, frame_skip=fs)
            raws = []
            inner = ex._get_raw_observation

            def spy():
                o = inner()
                raws.append(o)
                return o

            ex._get_raw_observation = spy
            res = ex.execute_replay(bytes(m), [int(b) for b in inp])
            assert len(res) == len(raws)
            return [(r["frame"], r["action"], o) for r, o in zip(res, raws)]

        run(*_probe_args())
        return "executor", run
    except Exception as e:   # noqa: BLE001 -- any failure to import or construct: the documented second way
        import traceback

        print("ReplayExecutor unavailable (%s: %s): driving NPlayHeadless in its loop\n%s"
              % (type(e).__name__, e, "".join(traceback.format_tb(e.__traceback__)[-3:])), flush=True)
    from nclone.nplay_headless import NPlayHeadless

    decode, to_action = _executor_file_functions()

    def run(m, inp, fs):
        hp = NPlayHeadless(render_mode="grayscale_array", enable_animation=False, enable_logging=False, enable_debug_overlay=False,
                           seed=42, enable_rendering=False)
        hp.load_map_from_map_data(list(bytes(m)))
        seq = [int(b) for b in inp]
        out = []
        for frame_idx, b in enumerate(seq):
            h, j = decode(b)
            hp.tick(h, j)
            if (frame_idx + 1) % max(1, fs) == 0:
                ns = hp.get_ninja_state()
                if not isinstance(ns, np.ndarray):
                    ns = np.array(ns, dtype=np.float32)
                current_frame = hp.sim.frame
                est = len(seq) or 2000
                tr = max(0.0, (est - current_frame) / est)
                x, y = hp.ninja_position()
                sx, sy = hp.exit_switch_position()
                dx, dy = hp.exit_door_position()
                out.append((frame_idx, to_action(b), {
                    "player_x": x, "player_y": y, "switch_x": sx, "switch_y": sy, "exit_door_x": dx, "exit_door_y": dy,
                    "switch_activated": hp.exit_switch_activated(), "game_state": np.append(ns[:40], tr).astype(np.float32),
                    "player_won": hp.ninja_has_won(), "player_dead": hp.sim.ninja.has_died()}))
        return out

    return "loop", run


def _probe_args():
    c = np.load(os.path.join(HERE, "corpus.npz"))
    return c["m3"], c["in3"][:2], 1


def main():
    c = np.load(os.path.join(HERE, "corpus.npz"))
    mode, run = make_runner()
    print("mode:", mode, flush=True)
    maps, inputs = [], []
    for r, i in enumerate(SRC):
        inp = np.array(c["in%d" % i], dtype=np.uint8)
        if r in CUT:
            inp = inp[:CUT[r]]
        maps.append(np.array(c["m%d" % i], dtype=np.uint8))
        inputs.append(inp)
    padded = np.zeros(len(SRC), dtype=np.uint8)

    def play_all():
        rows = {}
        for fs in FRAME_SKIPS:
            for r in range(len(SRC)):
                rows[fs, r] = run(maps[r], inputs[r], fs)
        return rows

    def after_win(rows):
        n = 0
        for (fs, r), rr in rows.items():
            won = [bool(o["player_won"]) for _, _, o in rr]
            n += sum(won[k] and won[k - 1] for k in range(1, len(won)))
        return n

    rows = play_all()
    if after_win(rows) == 0:
        inputs[0] = np.concatenate([inputs[0], np.zeros(PAD, dtype=np.uint8)])
        padded[0] = PAD
        print("no chosen replay continues past its win: %d NOOP bytes appended to entry 0 (corpus %d)" % (PAD, SRC[0]), flush=True)
        rows = play_all()
    out = {"mode": np.frombuffer(mode.encode(), dtype=np.uint8), "src": np.array(SRC, dtype=np.int32), "padded": padded,
           "fs": np.array(FRAME_SKIPS, dtype=np.int32)}
    for r in range(len(SRC)):
        out["m%d" % r], out["in%d" % r] = maps[r], inputs[r]
    for (fs, r), rr in rows.items():
        L = len(inputs[r])
        assert len(rr) == L // fs, (fs, r, len(rr), L)
        pre = "s%d_" % fs
        out[pre + "frame%d" % r] = np.array([f for f, _, _ in rr], dtype=np.int32)
        out[pre + "action%d" % r] = np.array([a for _, a, _ in rr], dtype=np.uint8)
        out[pre + "gs%d" % r] = np.array([np.asarray(o["game_state"], dtype=np.float32) for _, _, o in rr], dtype=np.float32).reshape(-1, 41)
        out[pre + "pos%d" % r] = np.array([[o["player_x"], o["player_y"], o["switch_x"], o["switch_y"], o["exit_door_x"], o["exit_door_y"]]
                                           for _, _, o in rr], dtype=np.float64).reshape(-1, 6)
        out[pre + "flags%d" % r] = np.array([(1 if o["player_won"] else 0) | (2 if o["player_dead"] else 0) | (4 if o["switch_activated"] else 0)
                                             for _, _, o in rr], dtype=np.uint8)
    # coverage
    n_after = after_win(rows)
    tail = [r for r in range(len(SRC)) if len(inputs[r]) % 4 != 0]
    empty = [(fs, r) for (fs, r), rr in rows.items() if len(rr) == 0]
    print("rows sampled after the win: %d; replays with L %% 4 != 0: %s; (fs, replay) with zero rows: %s" % (n_after, tail, empty))
    assert n_after >= 1 and tail and empty
    p = os.path.join(HERE, "demo.npz")
    _save_reproducible(p, out)
    print("demo.npz", os.path.getsize(p), "bytes, lengths", [len(x) for x in inputs])
    assert os.path.getsize(p) < 300 * 1024


def _save_reproducible(path, arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes."""
    import io
    import zipfile

    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


if __name__ == "__main__":
    main()
