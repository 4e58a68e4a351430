#!/usr/bin/env python3
"""Golden fixture for action routes: the list of actions the reference's env keeps per episode
(base_environment.py:186 `_action_sequence`, :517 append, :1677 clear) and the checkpoints built from it
(state_checkpoint.py StateCheckpoint), produced by RUNNING the reference.

Sibling of make_golden_minimal.py (same rules: build container only, never imported by the package, the tests, bench.py or
smoke(); the output is pure data).

    HOME=/tmp/orahome python3 tests/golden/make_golden_routes.py      # -> routes.npz

Levels and plans: five levels of minimal.npz with the 300-action plans that file already pins -- doors:replay:127, mines:replay:12,
mines:hcorr:mines:100001, c0:replay:0 and zoo:replay:6, whose plans contain 3, 5, 25, 13 and 4 episode ends (asserted).

Per level the plan is played on the reference's NPlayHeadless at frame_skip 4 (a step stops at the tick that ends the episode,
base_environment.py:524-609), with `reset()` (Simulator.reset) after a terminal step.  The running list is kept the way the env
keeps it: append per step, clear at reset.  At every 20th step that is not terminal a StateCheckpoint is built with
action_sequence, frame_count (sim.frame), ninja_position, ninja_velocity and switch_activated, and the reference's OWN
`ActionReplayer(frame_skip=4).replay_to_checkpoint` must accept it on a fresh simulator (its position validation on); its
velocity, frame count and switch state after that replay are asserted equal as well.  Nothing is restated: both classes are
imported from the reference as they stand.

Output routes.npz, per level k:
  m<k>    map_data f64; a<k> u8[300] the plan; t<k> u8[300] 1 where the step ended the episode
  cs<k>   i32[n] checkpoint step: the number of plan actions executed when the checkpoint was taken (20, 40, ...)
  cl<k>   i32[n] len(action_sequence): the route is a<k>[cs - cl : cs]
  cp<k>   f64[n, 2] ninja_position; cv<k> f64[n, 2] ninja_velocity; cw<k> u8[n] switch_activated; cf<k> i32[n] frame_count
names: newline-separated level tags.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LEVELS = ["doors:replay:127", "mines:replay:12", "mines:hcorr:mines:100001", "c0:replay:0", "zoo:replay:6"]
EPISODE_ENDS = [3, 5, 25, 13, 4]
EVERY = 20
FRAME_SKIP = 4


def main():
    sys.path.insert(0, HERE)
    import make_golden_reach as mgr

    mgr.prepare()
    from nclone.action_replayer import ActionReplayer
    from nclone.nplay_headless import NPlayHeadless
    from nclone.state_checkpoint import StateCheckpoint

    mini = np.load(os.path.join(HERE, "minimal.npz"))
    tags = bytes(mini["names"]).decode().split("\n")
    out = {}
    late = 0
    for k, tag in enumerate(LEVELS):
        src = tags.index(tag)
        m, plan, marks = mini["m%d" % src], mini["a%d" % src], mini["t%d" % src]
        assert int(marks.sum()) == EPISODE_ENDS[k] and EPISODE_ENDS[k] >= 2, (tag, int(marks.sum()))
        hp = NPlayHeadless(enable_rendering=False)
        hp.load_map_from_map_data(mgr.to_list(m))
        seq, T = [], []
        CS, CL, CP, CV, CW, CF = [], [], [], [], [], []
        first_end = None
        for s, a in enumerate(plan):
            h, j = mgr.ACTIONS[a]
            term = 0
            for _ in range(FRAME_SKIP):
                hp.tick(h, j)
                if hp.sim.ninja.state in (6, 7, 8):
                    term = 1
                    break
            seq.append(int(a))   # base_environment.py:517
            T.append(term)
            if term:
                if first_end is None:
                    first_end = s + 1
                hp.reset()
                seq.clear()      # base_environment.py:1677
                continue
            if (s + 1) % EVERY == 0:
                pos, vel = hp.ninja_position(), hp.ninja_velocity()
                ck = StateCheckpoint(cell=(int(pos[0] // 24), int(pos[1] // 24)), action_sequence=list(seq), frame_count=int(hp.sim.frame),
                                     ninja_position=(float(pos[0]), float(pos[1])), ninja_velocity=(float(vel[0]), float(vel[1])),
                                     switch_activated=bool(hp.exit_switch_activated()))
                fresh = NPlayHeadless(enable_rendering=False)
                fresh.load_map_from_map_data(mgr.to_list(m))
                res = ActionReplayer(validate_position=True, frame_skip=FRAME_SKIP).replay_to_checkpoint(fresh.sim, ck)
                assert res.success and res.position_error == 0.0, (tag, s + 1, res)
                assert tuple(fresh.ninja_velocity()) == ck.ninja_velocity and int(fresh.sim.frame) == ck.frame_count, (tag, s + 1)
                assert bool(fresh.exit_switch_activated()) == ck.switch_activated, (tag, s + 1)
                CS.append(s + 1); CL.append(len(ck.action_sequence)); CP.append(ck.ninja_position); CV.append(ck.ninja_velocity)
                CW.append(ck.switch_activated); CF.append(ck.frame_count)
                late += first_end is not None
        assert np.array_equal(np.array(T, dtype=np.uint8), marks), tag   # the plan plays as minimal.npz recorded it
        out["m%d" % k] = np.asarray(m, dtype=np.float64)
        out["a%d" % k] = np.asarray(plan, dtype=np.uint8)
        out["t%d" % k] = np.array(T, dtype=np.uint8)
        out["cs%d" % k] = np.array(CS, dtype=np.int32)
        out["cl%d" % k] = np.array(CL, dtype=np.int32)
        out["cp%d" % k] = np.array(CP, dtype=np.float64).reshape(-1, 2)
        out["cv%d" % k] = np.array(CV, dtype=np.float64).reshape(-1, 2)
        out["cw%d" % k] = np.array(CW, dtype=np.uint8)
        out["cf%d" % k] = np.array(CF, dtype=np.int32)
        print(k, tag, "episode ends", int(sum(T)), "checkpoints", len(CS), "route lengths", CL, flush=True)
    assert late >= 8, late   # checkpoints whose route is shorter than their step index
    out["names"] = np.frombuffer("\n".join(LEVELS).encode(), dtype=np.uint8)
    p = os.path.join(HERE, "routes.npz")
    np.savez_compressed(p, **out)
    print("routes.npz", os.path.getsize(p), "checkpoints after a first episode end:", late)


if __name__ == "__main__":
    main()
