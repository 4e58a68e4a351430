#!/usr/bin/env python3
"""Golden stacks of the reference's FrameStackWrapper (nclone/gym_environment/frame_stack_wrapper.py), produced by RUNNING the
wrapper on synthetic observation sequences (build container only).

gymnasium is not installed there, so a minimal `gymnasium` module is put into sys.modules first: the ObservationWrapper
base-class constructor (env, observation_space) and the Box / Dict containers -- nothing else.  frame_stack_wrapper.py is
loaded by file path (skipping the package __init__), so the wrapper's own reset(), observation() and
_reset_to_checkpoint_from_wrapper() run as written.  A step is what gymnasium's ObservationWrapper.step does: the inner env's
observation through wrapper.observation().

    NCLONE_SRC=<reference checkout> python3 tests/golden/make_golden_stack.py      # -> stack.npz

  events    i32[T]  per call: 0 step, 1 reset(), 2 _reset_to_checkpoint_from_wrapper()
  pf_in     u8[T, 84, 84, 1], gv_in u8[T, 176, 100, 1], gs_in f32[T, 41], am_in i8[T, 6]: the inner env's observations
  cfg       i32[C, 6]  per config: visual_stack_size, state_stack_size, padding (0 zero, 1 repeat), enable_visual_stacking,
                       enable_state_stacking, player_frame in the observation
  c<i>_pf   u8[T, ...] / c<i>_gs f32[T, ...]: the wrapper's player_frame / game_state after every call (absent without player_frame)
  c<i>_pass u8[T]     1 where global_view and action_mask came out unchanged
  c<i>_space_pf / c<i>_space_gs  f64[2 + ndim]: low, high, shape of the stacked observation space's Box; c<i>_space_dt u8[2]:
                       dtype codes (numpy .num) of those Boxes
  errors    the ValueError messages of the wrapper's argument checks, "\n"-joined bytes (visual 0, visual 13, state 0, state 13,
            padding "edge")
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.environ.get("NCLONE_SRC", "")   # a checkout of the reference nclone
T = 24
EVENTS = [1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0]   # resets at 0, 7, 21; a checkpoint reset at 11


def _shim():
    class Box:
        def __init__(self, low, high, shape=None, dtype=np.float32):
            self.low, self.high, self.shape, self.dtype = low, high, tuple(shape), np.dtype(dtype)

    class Dict:
        def __init__(self, spaces):
            self.spaces = dict(spaces)

    class ObservationWrapper:
        def __init__(self, env):
            self.env = env
            self.observation_space = env.observation_space

    gym = types.ModuleType("gymnasium")
    sp = types.ModuleType("gymnasium.spaces")
    sp.Box, sp.Dict = Box, Dict
    gym.spaces, gym.ObservationWrapper, gym.Env = sp, ObservationWrapper, object
    sys.modules["gymnasium"], sys.modules["gymnasium.spaces"] = gym, sp
    return Box, Dict


def _load_wrapper():
    path = os.path.join(SRC, "nclone", "gym_environment", "frame_stack_wrapper.py")
    spec = importlib.util.spec_from_file_location("frame_stack_wrapper", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.FrameStackWrapper


def _inputs():
    t = np.arange(T)
    ramp = np.arange(84 * 84, dtype=np.int64).reshape(84, 84, 1)
    pf = ((ramp[None] // 97 + 13 * t[:, None, None, None] + 1) % 251).astype(np.uint8)   # compressible, distinct per call
    gv = np.broadcast_to(((t * 5 + 3) % 256).astype(np.uint8)[:, None, None, None], (T, 176, 100, 1)).copy()
    rng = np.random.default_rng(7)
    gs = rng.uniform(-1, 1, size=(T, 41)).astype(np.float32)
    am = rng.integers(0, 2, size=(T, 6)).astype(np.int8)
    return pf, gv, gs, am


class _Inner:
    """The wrapped env: hands out the prepared observation of call i."""

    def __init__(self, Box, Dict, pf, gv, gs, am, with_pf):
        self.pf, self.gv, self.gs, self.am, self.with_pf, self.i = pf, gv, gs, am, with_pf, 0
        sp = {"game_state": Box(-1.0, 1.0, (41,), np.float32), "action_mask": Box(0, 1, (6,), np.int8)}
        if with_pf:
            sp["player_frame"] = Box(0, 255, (84, 84, 1), np.uint8)
            sp["global_view"] = Box(0, 255, (176, 100, 1), np.uint8)
        self.observation_space = Dict(sp)

    def obs(self):
        o = {"game_state": self.gs[self.i].copy(), "action_mask": self.am[self.i].copy()}
        if self.with_pf:
            o["player_frame"] = self.pf[self.i].copy()
            o["global_view"] = self.gv[self.i].copy()
        return o

    def reset(self, **kw):
        return self.obs(), {}

    def _reset_to_checkpoint_from_wrapper(self, checkpoint):
        return self.obs(), {}


def configs():
    out = []
    for k, ks in ((1, 12), (2, 4), (4, 2), (12, 1)):
        for pad in (0, 1):
            out.append((k, ks, pad, 1, 1, 1))
    out += [(4, 4, 0, 1, 0, 1), (4, 4, 1, 0, 1, 1), (4, 4, 0, 0, 0, 1), (3, 4, 1, 1, 1, 0), (12, 12, 1, 1, 1, 1)]
    return out


def main():
    if not os.path.isdir(os.path.join(SRC, "nclone")):
        sys.exit("set NCLONE_SRC to a checkout of the reference nclone")
    Box, Dict = _shim()
    FrameStackWrapper = _load_wrapper()
    pf, gv, gs, am = _inputs()
    res = {"events": np.array(EVENTS, dtype=np.int32), "pf_in": pf, "gv_in": gv, "gs_in": gs, "am_in": am}
    cfgs = configs()
    res["cfg"] = np.array(cfgs, dtype=np.int32)
    for c, (vk, sk, pad, ven, sen, with_pf) in enumerate(cfgs):
        inner = _Inner(Box, Dict, pf, gv, gs, am, with_pf)
        w = FrameStackWrapper(inner, visual_stack_size=vk, state_stack_size=sk, enable_visual_stacking=bool(ven),
                              enable_state_stacking=bool(sen), padding_type=("zero", "repeat")[pad])
        pfo, gso, ok = [], [], []
        for i, ev in enumerate(EVENTS):
            inner.i = i
            if ev == 1:
                o, _ = w.reset()
            elif ev == 2:
                o, _ = w._reset_to_checkpoint_from_wrapper(object())
            else:
                o = w.observation(inner.obs())
            gso.append(np.asarray(o["game_state"]))
            same = np.array_equal(o["action_mask"], am[i])
            if with_pf:
                pfo.append(np.asarray(o["player_frame"]))
                same = same and np.array_equal(o["global_view"], gv[i])
            ok.append(same)
        res["c%d_gs" % c] = np.stack(gso)
        if with_pf:
            res["c%d_pf" % c] = np.stack(pfo)
        res["c%d_pass" % c] = np.array(ok, dtype=np.uint8)
        for key, name in (("player_frame", "pf"), ("game_state", "gs")):
            if key in w.observation_space.spaces:
                b = w.observation_space.spaces[key]
                res["c%d_space_%s" % (c, name)] = np.array([b.low, b.high] + list(b.shape), dtype=np.float64)
        res["c%d_space_dt" % c] = np.array([w.observation_space.spaces[k].dtype.num if k in w.observation_space.spaces else 0
                                            for k in ("player_frame", "game_state")], dtype=np.uint8)
    errs = []
    for kw in ({"visual_stack_size": 0}, {"visual_stack_size": 13}, {"state_stack_size": 0}, {"state_stack_size": 13},
               {"padding_type": "edge"}):
        try:
            FrameStackWrapper(_Inner(Box, Dict, pf, gv, gs, am, 1), **kw)
            errs.append("")
        except ValueError as e:
            errs.append(str(e))
    res["errors"] = np.frombuffer("\n".join(errs).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(HERE, "stack.npz"), **res)
    print("stack.npz: %d configs x %d calls" % (len(cfgs), T))


if __name__ == "__main__":
    main()
