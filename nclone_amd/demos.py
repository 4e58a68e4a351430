"""Demonstration transitions from recorded replays, played as one batch on the GPU.

Counterpart of the reference's behavioural-cloning data path: ReplayExecutor.execute_replay (nclone/replay/replay_executor.py:304-462)
plays one replay at a time in Python and DemonstrationBuffer (nclone/replay/demonstration_buffer.py:72-209) turns the result into
(observation, action, done) transitions behind a process pool and an on-disk .npz cache.  Here `load_demonstrations` plays R replays
over N envs through npp_demo_create / npp_demo_play (include/npp_amd.h) and returns the packed dataset as device
tensors: no cache to invalidate when the observation space changes.

Deliberate deviation: reachability_features, spatial_context, switch_states and mine_sdf_features are the rows this project's env
path produces for the state (pinned against the reference's env), not the executor's private re-implementations.  game_state[40]
IS the executor's time value, and action_mask its all ones unless action_mask="env".
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _native as nat
from .engine import NppBatch, reach_level_info
from .replay import CompactReplay

# the vector keys of the reference's DEFAULT_OBSERVATION_KEYS (demonstration_buffer.py:49-60); its graph keys are per level: the
# dataset carries a `level` column and NppBatch.graph_observation / engine.graph_tables serve the per-level tables
DEFAULT_OBSERVATION_KEYS = ("game_state", "reachability_features", "switch_states", "action_mask", "spatial_context", "mine_sdf_features")
OBSERVATION_KEYS = {"game_state": (41, torch.float32), "action_mask": (6, torch.int8), "entity_positions": (6, torch.float32),
                    "spatial_context": (112, torch.float32), "reachability_features": (38, torch.float32),
                    "mine_sdf_features": (3, torch.float32), "switch_states": (25, torch.float32)}
COLUMNS = {"positions": (6, torch.float64), "action": (None, torch.uint8), "frame": (None, torch.int32), "done": (None, torch.uint8),
           "replay": (None, torch.int32), "level": (None, torch.int32), "flags": (None, torch.uint8), "status": (None, torch.int32)}
_REACH_KEYS = ("reachability_features", "mine_sdf_features")
STATUS_LEVEL_REFUSED = 2   # `status` of rows whose level npp_reachability refuses (npp_reach_features_host's bit 1)


def plan(lengths, frame_skip, max_transitions, n_envs):
    """npp_demo_plan_host: {"rows" i32[R], "row_base" i64[R], "order" (the scheduled replays, longest first), "round_ticks" (ticks per
    round), "rows_total"}; ValueError where the native plan refuses."""
    L = nat.lib()
    ln = np.ascontiguousarray(lengths, dtype=np.int64)
    n = len(ln)
    rows, base = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int64)
    order, ticks = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    counts, total = np.zeros(2, dtype=np.int32), np.zeros(1, dtype=np.int64)
    p = [a.ctypes.data_as(C.c_void_p) for a in (ln, rows, base, order, ticks, counts, total)]
    rc = L.npp_demo_plan_host(p[0], n, int(frame_skip), int(max_transitions), int(n_envs), *p[1:])
    if rc != nat.NPP_OK:
        raise ValueError((L.npp_last_error(None) or b"npp_demo_plan_host failed").decode())
    return {"rows": rows, "row_base": base, "order": order[:counts[0]].copy(), "round_ticks": ticks[:counts[1]].copy(),
            "rows_total": int(total[0])}


def _as_replay(r):
    if isinstance(r, CompactReplay):
        return r
    with open(os.fspath(r), "rb") as f:
        return CompactReplay.from_binary(f.read())


def _served_keys(observation_keys):
    """The keys asked for, in the canonical order; ValueError for one that is not served."""
    unknown = [k for k in observation_keys if k not in OBSERVATION_KEYS]
    if unknown:
        raise ValueError("unknown observation keys %s (served: %s)" % (unknown, ", ".join(OBSERVATION_KEYS)))
    return tuple(k for k in OBSERVATION_KEYS if k in observation_keys)


def _shape(rows, dim):
    return (rows,) + (() if dim is None else (dim,))


class DemoPlayer:
    """The player behind load_demonstrations: owns a private NppBatch (auto-reset off; a user's vec env is never touched), the
    de-duplicated level set and the native demo object.  `play(planes)` fills caller-allocated tensors."""

    def __init__(self, replays, frame_skip=1, max_transitions_per_demo=10_000, observation_keys=DEFAULT_OBSERVATION_KEYS, n_envs=None,
                 device=0, action_mask="ones"):
        if action_mask not in ("ones", "env"):
            raise ValueError('action_mask must be "ones" or "env"')
        self.keys = _served_keys(observation_keys)
        self.replays = list(replays)
        if not self.replays:
            raise ValueError("no replays to play")
        self.frame_skip, self.cap = int(frame_skip), int(max_transitions_per_demo)
        ids, self.levels = {}, []
        self.level_ids = np.zeros(len(self.replays), dtype=np.int32)
        for i, r in enumerate(self.replays):   # maps are de-duplicated: one level per distinct map
            if r.map_data not in ids:
                ids[r.map_data] = len(self.levels)
                self.levels.append(np.frombuffer(r.map_data, dtype=np.uint8))
            self.level_ids[i] = ids[r.map_data]
        self.lengths = np.array([len(r.input_sequence) for r in self.replays], dtype=np.int64)
        self.n_envs = int(n_envs) if n_envs is not None else max(1, min(len(self.replays), 4096))
        self.plan = plan(self.lengths, self.frame_skip, self.cap, self.n_envs)   # (refuses bad arguments before a handle exists)
        self.rows_total = self.plan["rows_total"]
        self.batch = NppBatch(self.n_envs, device=device, autoreset=False)
        self.device = self.batch.device
        try:
            self._create(action_mask)
        except Exception:
            self.batch.close()   # a refused level set or demo object leaves no handle behind
            raise

    def _create(self, action_mask):
        self.batch.load_levels(self.levels)
        offsets = np.zeros(len(self.replays) + 1, dtype=np.int64)
        np.cumsum(self.lengths, out=offsets[1:])
        table = np.zeros(max(int(offsets[-1]), 1), dtype=np.uint8)
        for i, r in enumerate(self.replays):
            table[offsets[i]:offsets[i + 1]] = np.asarray(r.input_sequence, dtype=np.uint8)
        self.key_flags = sum(nat.DEMO_KEY_FLAGS[k] for k in self.keys) | nat.DEMO_KEY_FLAGS["positions"]
        if action_mask == "env":
            self.key_flags |= nat.DEMO_MASK_ENV
        b = self.batch
        with b._ctx():
            nat.check(b.h, b.lib.npp_demo_create(b.h, table.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.c_void_p),
                                                 self.level_ids.ctypes.data_as(C.c_void_p), len(self.replays), self.frame_skip, self.cap,
                                                 self.key_flags))

    def allocate(self, guard=0, fill=None):
        """{name: tensor [guard + rows_total + guard, dim]} for every key and column, zeroed or filled with `fill`."""
        out = {}
        with self.batch._ctx():
            for k, (dim, dt) in list(OBSERVATION_KEYS.items()) + list(COLUMNS.items()):
                if k in OBSERVATION_KEYS and k not in self.keys:
                    continue
                shape = (self.rows_total + 2 * guard,) + (() if dim is None else (dim,))
                out[k] = torch.zeros(shape, dtype=dt, device=self.device) if fill is None else torch.full(shape, fill, dtype=dt, device=self.device)
        return out

    def play(self, planes):
        """Fill `planes` ({name: contiguous device tensor [rows_total, dim]}; every key of the player must be there, columns are
        optional).  Asynchronous on the batch's stream."""
        if self.rows_total == 0:
            return
        o = nat.DemoOut()
        for k, (dim, dt) in list(OBSERVATION_KEYS.items()) + list(COLUMNS.items()):
            t = planes.get(k)
            if t is None:
                if k in self.keys or k == "positions":
                    raise ValueError("no destination for key %r" % k)
                continue
            want = (self.rows_total,) + (() if dim is None else (dim,))
            if tuple(t.shape) != want or t.dtype != dt or not t.is_contiguous() or t.device != self.device:
                raise ValueError("plane %r must be a contiguous %s tensor of shape %s on %s" % (k, dt, want, self.device))
            setattr(o, "d_" + k, t.data_ptr())
        b = self.batch
        with b._ctx():
            nat.check(b.h, b.lib.npp_demo_play(b.h, C.byref(o)))

    def close(self):
        self.batch.close()


class DemonstrationSet:
    """The packed transitions of a replay set: replay-major in the order of the played replays, time-ordered inside a replay.

    observations   {key: tensor [rows, dim]} on the device
    action u8, done u8, frame i32 (the tick the row was sampled after), replay i32 (index into the `replays` argument of
    load_demonstrations), level i32 (index into `levels`), flags u8 (1 won | 2 dead | 4 exit switch), positions f64 [rows, 6],
    status i32, valid = status == 0 (rows of a level npp_reachability refuses carry zero reachability rows and status 2)
    """

    def __init__(self, observations, columns, replay_index, rows, levels, frame_skip):
        self.observations = observations
        for k, v in columns.items():
            setattr(self, k, v)
        self.valid = self.status == 0
        self.replay_index = np.asarray(replay_index, dtype=np.int64)   # the played replays, as indices into the caller's list
        self.rows = np.asarray(rows, dtype=np.int64)                   # rows of each played replay
        self.row_base = np.concatenate([[0], np.cumsum(self.rows)[:-1]]).astype(np.int64) if len(self.rows) else np.zeros(0, dtype=np.int64)
        self.levels = levels
        self.frame_skip = frame_skip
        self._valid_idx = None

    def __len__(self):
        return int(self.action.shape[0])

    def actions(self, dtype=torch.int64):
        return self.action.to(dtype)

    def episode_slices(self):
        """One slice of rows per played replay (empty for a replay shorter than the frame skip); row i + 1 of a slice is the
        next_observation of row i."""
        return [slice(int(b), int(b + r)) for b, r in zip(self.row_base, self.rows)]

    def sample_batch(self, batch_size, generator=None):
        """{"observations": {key: [B, dim]}, "actions": i64 [B], "indices": i64 [B]}: uniform over the valid rows, one index_select
        per key.  `generator`: a torch.Generator (on the CPU or on the set's device)."""
        if self._valid_idx is None:
            self._valid_idx = torch.nonzero(self.valid, as_tuple=False).flatten()
        n = int(self._valid_idx.numel())
        if n == 0:
            raise ValueError("the demonstration set has no valid row")
        dev = self.action.device
        gdev = generator.device if generator is not None else dev
        pick = torch.randint(0, n, (int(batch_size),), generator=generator, device=gdev).to(dev)
        idx = self._valid_idx.index_select(0, pick)
        return {"observations": {k: v.index_select(0, idx) for k, v in self.observations.items()},
                "actions": self.action.index_select(0, idx).to(torch.int64), "indices": idx}

    def to_numpy(self):
        out = {k: v.cpu().numpy() for k, v in self.observations.items()}
        for k in COLUMNS:
            out[k] = getattr(self, k).cpu().numpy()
        out["valid"] = self.valid.cpu().numpy()
        return out


def load_demonstrations(replays, frame_skip=1, max_transitions_per_demo=10_000, observation_keys=DEFAULT_OBSERVATION_KEYS, n_envs=None,
                        device=0, action_mask="ones"):
    """DemonstrationBuffer's data for a set of replays (CompactReplay objects or paths of .replay files), under the observation
    keys asked for.  Failures (success byte 0) are skipped as demonstration_buffer.py:125-127 does.  n_envs: envs of the private
    player (default: one per played replay, at most 4096): R replays over N envs take ceil(R / N) rounds, each as long as its
    longest replay."""
    reps = [_as_replay(r) for r in replays]
    kept = [i for i, r in enumerate(reps) if r.success]
    keys = _served_keys(observation_keys)
    dev = torch.device("cuda", int(device))
    if not kept:
        obs = {k: torch.zeros(_shape(0, OBSERVATION_KEYS[k][0]), dtype=OBSERVATION_KEYS[k][1], device=dev) for k in keys}
        cols = {k: torch.zeros(_shape(0, d), dtype=t, device=dev) for k, (d, t) in COLUMNS.items()}
        return DemonstrationSet(obs, cols, [], [], [], int(frame_skip))
    # a level npp_reachability refuses: its replays are played without the reachability keys and keep zero rows there
    refused = {}
    if any(k in keys for k in _REACH_KEYS):
        for i in kept:
            m = reps[i].map_data
            if m not in refused:
                refused[m] = not reach_level_info(np.frombuffer(m, dtype=np.uint8))["supported"]
    groups = [([i for i in kept if not refused.get(reps[i].map_data, False)], keys, 0),
              ([i for i in kept if refused.get(reps[i].map_data, False)], tuple(k for k in keys if k not in _REACH_KEYS), STATUS_LEVEL_REFUSED)]
    parts, levels, level_of = [], [], {}
    for idx, gkeys, status in groups:
        if not idx:
            continue
        pl = DemoPlayer([reps[i] for i in idx], frame_skip, max_transitions_per_demo, gkeys, n_envs, device, action_mask)
        try:
            planes = pl.allocate()
            pl.play(planes)
            pl.batch.sync()
        finally:
            pl.close()
        lut = []
        for m in pl.levels:   # the set's levels: distinct maps over all groups
            key = m.tobytes()
            if key not in level_of:
                level_of[key] = len(levels)
                levels.append(m)
            lut.append(level_of[key])
        planes["level"] = torch.as_tensor(lut, dtype=torch.int32, device=dev)[planes["level"].long()]
        planes["replay"] = torch.as_tensor(idx, dtype=torch.int32, device=dev)[planes["replay"].long()]
        if status:
            planes["status"].fill_(status)
        for k in keys:   # the keys this group was played without: zero rows
            if k not in planes:
                planes[k] = torch.zeros(_shape(pl.rows_total, OBSERVATION_KEYS[k][0]), dtype=OBSERVATION_KEYS[k][1], device=dev)
        parts.append((idx, pl.plan["rows"], planes))
    if len(parts) == 1:
        order, row_counts, planes = parts[0]
    else:   # the groups' rows, one after the other, gathered into the caller's order (replay-major)
        seq = sorted((i, g, j) for g, (idx, _, _) in enumerate(parts) for j, i in enumerate(idx))
        order = [i for i, _, _ in seq]
        row_counts = [int(parts[g][1][j]) for _, g, j in seq]
        starts, at = [], 0
        for _, rows, _ in parts:   # first row of every replay in the concatenation
            starts.append(at + np.concatenate([[0], np.cumsum(rows)[:-1]]))
            at += int(np.sum(rows))
        pick = np.concatenate([np.arange(starts[g][j], starts[g][j] + n) for (_, g, j), n in zip(seq, row_counts)]).astype(np.int64)
        pick = torch.from_numpy(pick).to(dev)
        planes = {k: torch.cat([p[2][k] for p in parts], 0).index_select(0, pick) for k in list(keys) + list(COLUMNS)}
    obs = {k: planes[k] for k in keys}
    cols = {k: planes[k] for k in COLUMNS}
    return DemonstrationSet(obs, cols, order, row_counts, levels, int(frame_skip))
