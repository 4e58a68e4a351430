"""NppBatch: the thin host object over one native handle (N environments on one GPU).

PyTorch is used only as plumbing: device buffers for actions/observations and the HIP stream.  All
simulation work happens in the HIP kernels behind the C ABI (include/npp_amd.h).
"""
import ctypes as C

import numpy as np
import torch

from . import _native as nat
from .spaces import check_frame_augmentation


class _DeviceStream:
    """torch.cuda.device + torch.cuda.stream in one context manager."""

    def __init__(self, device, stream):
        self._d = torch.cuda.device(device)
        self._s = torch.cuda.stream(stream)

    def __enter__(self):
        self._d.__enter__()
        self._s.__enter__()

    def __exit__(self, *a):
        self._s.__exit__(*a)
        self._d.__exit__(*a)


def _as_f64_blob(levels):
    """levels: sequence of 1-D arrays/lists/bytes of raw map_data values -> (blob f64, offsets i64)."""
    arrs = []
    for m in levels:
        if isinstance(m, (bytes, bytearray)):
            m = np.frombuffer(bytes(m), dtype=np.uint8)
        arrs.append(np.ascontiguousarray(np.asarray(m, dtype=np.float64).ravel()))
    offsets = np.zeros(len(arrs) + 1, dtype=np.int64)
    for i, a in enumerate(arrs):
        offsets[i + 1] = offsets[i] + len(a)
    blob = np.concatenate(arrs) if arrs else np.zeros(0, dtype=np.float64)
    return blob, offsets


# every output the kernels can produce: name -> (per-env shape, dtype).  The first six are the packed observation block
# of BASELINE.json config 4 (what a learner on another GPU needs each step); they sit first and contiguous in the block.
_FIELDS = {
    "game_state": ((41,), torch.float32),
    "entity_pos": ((6,), torch.float32),
    "reward": ((), torch.float32),
    "frames": ((), torch.int16),
    "action_mask": ((6,), torch.int8),
    "flags": ((), torch.uint8),
    "terminal_state": ((41,), torch.float32),
    "spatial_context": ((112,), torch.float32),
    "positions": ((6,), torch.float64),
    "work": ((), torch.int16),
    "switch_states": ((25,), torch.float32),
    "player_frame": ((84, 84, 1), torch.uint8),
    "global_view": ((176, 100, 1), torch.uint8),
    "reachability_features": ((38,), torch.float32),
    "mine_sdf_features": ((3,), torch.float32),
    "reach_status": ((), torch.int32),
    "minimal_observation": ((40,), torch.float32),
    "path_direction": ((), torch.int8),
    "reward_components": ((6,), torch.float32),
}
# graph observations (NppBatch.graph_observation): shape per env and dtype; kept out of the packed output block, which numpy-mode
# environments copy to the host every step
GRAPH_KEYS = {"graph_node_feats": ((2500, 6), torch.float32), "graph_edge_index": ((2, 20000), torch.uint16),
              "graph_node_mask": ((2500,), torch.uint8), "graph_edge_mask": ((20000,), torch.uint8)}
_ALWAYS = ("game_state", "entity_pos", "reward", "frames", "action_mask", "flags", "terminal_state")
_PACKED = ("game_state", "entity_pos", "reward", "frames", "action_mask", "flags")
_OPTIONAL = ("spatial_context", "positions", "work", "switch_states", "player_frame", "global_view", "reachability_features",
             "mine_sdf_features", "reach_status", "minimal_observation", "path_direction", "reward_components")
REWARD_COMPONENTS = ("pbrs", "distance_milestone", "switch_milestone", "approach_bonus", "terminal", "potential")
REWARD_PARAMS = ("death_penalty", "level_completion_reward", "switch_activation_reward", "time_penalty_per_step", "pbrs_objective_weight",
                 "pbrs_gamma")
WAYPOINT_PARAMS = ("collection_radius", "out_of_order_scale", "progress_scale", "progress_spacing")


AUG_SCALES = {"light": 0.7, "medium": 1.0, "strong": 1.3}   # frame_augmentation.py:57
AUG_WORDS = 14   # int32 words of one AugParams (npp_augment.hpp)


def check_archive_lists(envs, slots, unique, what):
    """The host-side checks of NppBatch.archive_store / archive_restore (no device needed): both lists one-dimensional, of one
    length, int32 when they are tensors and integers when they are arrays; in an array, no value of the `unique` list ("envs" or
    "slots") comes twice among the entries that are not skipped.  CUDA tensors are taken as they are -- no host copy, no
    synchronisation: the device decides every entry.  Returns {"envs": ..., "slots": ...} with arrays as numpy arrays."""
    lists = {"envs": envs, "slots": slots}
    for name, v in lists.items():
        if isinstance(v, torch.Tensor):
            if v.dtype != torch.int32:
                raise TypeError("%s: %s must be an int32 tensor, not %s" % (what, name, v.dtype))
        else:
            v = lists[name] = np.asarray(v)
            if v.dtype.kind not in "iu":
                raise TypeError("%s: %s must hold integers, not %s" % (what, name, v.dtype))
        if v.ndim != 1:
            raise ValueError("%s: %s must be one-dimensional" % (what, name))
    if len(lists["envs"]) != len(lists["slots"]):
        raise ValueError("%s: envs and slots differ in length (%d, %d)" % (what, len(lists["envs"]), len(lists["slots"])))
    u, other = lists[unique], lists["slots" if unique == "envs" else "envs"]
    if isinstance(u, np.ndarray):
        live = u[(u >= 0) & (other >= 0)] if isinstance(other, np.ndarray) else u[u >= 0]
        if len(np.unique(live)) != len(live):
            raise ValueError("%s: the same %s comes twice" % (what, unique[:-1]))
    return lists


CELLS_PER_LEVEL = 2 * 25 * 44   # keys of the cell index per level: (switch_activated, cell_y, cell_x)


def check_cell_arg(v, dtype, n, what):
    """The host-side checks of a per-env argument of NppBatch.archive_explore / archive_select (no device needed): one value per
    env; a tensor must have the dtype the kernel reads (bool counts as uint8), an array is converted.  Returns the tensor (bool
    viewed as uint8) or a contiguous numpy array of that dtype."""
    np_dtype = {torch.float32: np.float32, torch.uint8: np.uint8}[dtype]
    if isinstance(v, torch.Tensor):
        if v.dtype == torch.bool and dtype == torch.uint8:
            v = v.view(torch.uint8)
        if v.dtype != dtype:
            raise TypeError("%s must be a %s tensor, not %s" % (what, str(dtype).replace("torch.", ""), v.dtype))
    else:
        v = np.ascontiguousarray(v, dtype=np_dtype)
    if v.ndim != 1 or len(v) != n:
        raise ValueError("%s must be [%d] (one value per env)" % (what, n))
    return v


def _device_tensor(ptr, numel, dtype, device):
    """A torch tensor over `numel` elements of device memory that the native handle owns (no copy, no ownership)."""
    typestr = {torch.uint8: "|u1", torch.float32: "<f4", torch.int32: "<i4", torch.float64: "<f8", torch.int64: "<i8"}[dtype]

    class _Holder:
        __cuda_array_interface__ = {"shape": (int(numel),), "typestr": typestr, "data": (int(ptr), False), "version": 2}

    return torch.as_tensor(_Holder(), device=device)


class OutputBlock:
    """All enabled outputs of one handle in ONE contiguous device allocation (each field 256-byte aligned), plus two pinned
    host mirrors.  One block means: one RCCL all_gather moves the whole packed observation of a rank (config 4), and one
    asynchronous device-to-host copy + one synchronisation serves a numpy training loop (`to_host`)."""

    def __init__(self, n, device, names):
        self.n = int(n)
        self.names = [k for k in _FIELDS if k in names]   # canonical order: packed observation first
        self.offsets = {}
        off = 0
        for k in self.names:
            shape, dt = _FIELDS[k]
            nbytes = self.n * int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dt).element_size()
            self.offsets[k] = (off, nbytes)
            off = (off + nbytes + 255) // 256 * 256
            if k == _PACKED[-1]:
                self.packed_bytes = off
        self.nbytes = off
        self.dev = torch.zeros(self.nbytes, dtype=torch.uint8, device=device)
        self.t = {k: self._view(self.dev, k) for k in self.names}
        self._host = [None, None]
        self._flip = 0

    def _view(self, base, k):
        off, nbytes = self.offsets[k]
        shape, dt = _FIELDS[k]
        return base[off:off + nbytes].view(dt).view((self.n,) + tuple(shape))

    def packed(self):
        """uint8 view of the packed observation (game_state, entity_pos, reward, frames, action_mask, flags)."""
        return self.dev[:self.packed_bytes]

    def split_packed(self, gathered, world):
        """Views into an all-gathered [world * packed_bytes] uint8 tensor: {name: [world, n, ...]}."""
        g = gathered.view(world, self.packed_bytes)
        out = {}
        for k in _PACKED:
            off, nbytes = self.offsets[k]
            shape, dt = _FIELDS[k]
            out[k] = g[:, off:off + nbytes].contiguous().view(dt).view((world, self.n) + tuple(shape))
        return out

    def to_host(self, stream, names=None):
        """One async copy of the block (from the first to the last requested field) into a pinned mirror on `stream`, one
        synchronisation; returns {name: numpy view}.  Two mirrors alternate, so the arrays of the previous call stay valid
        until the call after this one (obs_t and obs_t+1 can be held together)."""
        names = self.names if names is None else [k for k in self.names if k in names]
        start = min(self.offsets[k][0] for k in names)   # (fields start 256-byte aligned) nothing in front of the first one asked for
        end = max(self.offsets[k][0] + self.offsets[k][1] for k in names)
        if self._host[self._flip] is None:
            self._host[self._flip] = torch.empty(self.nbytes, dtype=torch.uint8, pin_memory=True)
        host = self._host[self._flip]
        self._flip ^= 1
        with torch.cuda.stream(stream):
            host[start:end].copy_(self.dev[start:end], non_blocking=True)
        stream.synchronize()
        return {k: self._view(host, k).numpy() for k in names}


class NppBatch:
    """N environments stepped in lock-step on one GPU.

    Counterpart of N instances of the reference's NPlayHeadless (nclone/nplay_headless.py:28).
    """

    def __init__(self, n_envs, device=0, autoreset=True, allow_unsupported=False, frame_centered=False, stream=None,
                 outputs=(), fast_reset=False):
        self.lib = nat.lib()
        if not torch.cuda.is_available():
            raise RuntimeError("nclone_amd needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU fallback")
        self.n = int(n_envs)
        self.device = torch.device("cuda", int(device))
        flags = ((nat.FLAG_AUTORESET if autoreset else 0) | (nat.FLAG_ALLOW_UNSUPPORTED if allow_unsupported else 0)
                 | (nat.FLAG_FRAME_CENTERED if frame_centered else 0) | (nat.FLAG_FAST_RESET if fast_reset else 0))
        h = C.c_void_p()
        nat.check(None, self.lib.npp_create(self.n, int(device), flags, C.byref(h)))
        self.h = h
        self.n_levels = 0
        with torch.cuda.device(self.device):
            # every launch of this handle is ordered on ONE HIP stream; handles on different streams overlap on the GPU
            self.stream = stream if stream is not None else torch.cuda.current_stream()
            nat.check(self.h, self.lib.npp_set_stream(self.h, C.c_void_p(self.stream.cuda_stream)))
        self._enabled = set(_ALWAYS)
        self._masking = 0         # action masking mode (set_action_masking)
        self._mask_stats = None   # views of the handle's counters (path_mask_stats): the handle's own buffers, alive as long as it is
        self._reward_mode = 0     # 0 sparse, 1 pbrs (set_reward_mode)
        self._reward_pending = False   # a step() ran whose step_reward() has not: the handle holds that step's flags / frames rows
        self._reward_waypoints = False   # set_reward_waypoints
        for k in outputs:
            if k not in _OPTIONAL:
                raise ValueError("unknown output %r (optional outputs: %s)" % (k, ", ".join(_OPTIONAL)))
            self._enabled.add(k)
        self._build_block()

    def _build_block(self):
        self._reward_pending = False   # (the rows of the last step may have been in the old block)
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            self.out = OutputBlock(self.n, self.device, self._enabled)
        t = self.out.t
        self.game_state, self.action_mask, self.entity_pos = t["game_state"], t["action_mask"], t["entity_pos"]
        self.flags, self.reward, self.frames, self.terminal_state = t["flags"], t["reward"], t["frames"], t["terminal_state"]
        self.spatial_context = t.get("spatial_context")
        self.positions = t.get("positions")
        self.work = t.get("work")

        def ptr(k):
            return t[k].data_ptr() if k in t else None

        self._out = nat.StepOut(ptr("game_state"), ptr("action_mask"), ptr("entity_pos"), ptr("flags"), ptr("reward"),
                                ptr("frames"), ptr("terminal_state"), ptr("spatial_context"), ptr("positions"), ptr("work"))
        self._out_min = nat.StepOut(ptr("game_state"), ptr("action_mask"), ptr("entity_pos"), ptr("flags"), ptr("reward"),
                                    ptr("frames"), None, ptr("spatial_context"), ptr("positions"), ptr("work"))
        if "minimal_observation" in t:
            # the mode's switch: from now on every step / observe launch writes the mine rows the 40 floats are assembled from
            # (into spatial_context when that output is enabled, else into a buffer of the handle).  Called again whenever the
            # block is re-allocated: the handle forgets where the last launch wrote the rows (they may have been in the old block),
            # so a minimal_observation() before the next step() / observe() is an error instead of a read of freed memory
            nat.check(self.h, self.lib.npp_set_minimal_observation(self.h, 1))

    def enable_outputs(self, *names):
        """Add optional outputs (spatial_context, positions, work, switch_states, player_frame, global_view, reachability_features, mine_sdf_features, reach_status, minimal_observation, path_direction, reward_components); the output
        block is re-allocated, so tensors obtained earlier are stale."""
        new = [k for k in names if k not in self._enabled]
        for k in new:
            if k not in _OPTIONAL:
                raise ValueError("unknown output %r" % (k,))
            self._enabled.add(k)
        if new:
            self._build_block()

    def enable_spatial_context(self):
        """Also produce the 112-float spatial_context observation (8x8 tile categories + 8 nearest mines)."""
        self.enable_outputs("spatial_context")

    def _ctx(self):
        """Launches, copies and allocations of this handle run with its device current and on its stream."""
        return _DeviceStream(self.device, self.stream)

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.lib.npp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- levels -----------------------------------------------------------------------------------------------
    def load_levels(self, levels):
        blob, offsets = _as_f64_blob(levels)
        nat.check(self.h, self.lib.npp_load_levels(
            self.h, blob.ctypes.data_as(C.POINTER(C.c_double)), offsets.ctypes.data_as(C.POINTER(C.c_int64)), len(offsets) - 1))
        self.n_levels = len(offsets) - 1
        self._archive_meta = self._archive_cells = self._archive_route_views = None   # (the checkpoint archive and its cell index go with the level set)
        self._episode_views = None   # (so do the episode statistics: the table has a row per level)
        self._reward_mode, self._reward_pending = 0, False   # (so does reward mode "pbrs": its constants are per level)
        self._reward_waypoints = False
        self._goal = None   # (and the goal curriculum: its variants were compiled from the old set)
        self._sweep = None  # (and an evaluation sweep with its results: the jobs named levels of the old set)

    # ---- goal curriculum (include/npp_amd.h npp_set_goal_curriculum; the reference's IntermediateGoalManager) -----
    GOAL_LEVEL_WORDS = ("stage", "pending", "num_stages", "variant0", "fill", "head", "wins", "advances", "appended", "stale")
    GOAL_ENV_WORDS = ("episode_count", "switch_activation_count", "completion_count", "switch_seen", "level_at_end")

    def set_goal_curriculum(self, on=True, stage_distance_interval=100.0, advancement_threshold=0.80, rolling_window=500,
                            auto_advance=True):
        """Switch the goal curriculum on or off.  Switching RELOADS the level set (base levels + one variant level per stage), as
        load_levels does: the pool, the archive, the reward mode and the episode statistics go off, so call it first.  Every env
        restarts on the stage-0 variant of the base level it played.  Bad numbers raise ValueError with the native message."""
        q = nat.GoalCurriculumParams(float(stage_distance_interval), float(advancement_threshold), int(rolling_window),
                                     1 if auto_advance else 0)
        code = self.lib.npp_set_goal_curriculum(self.h, 1 if on else 0, C.byref(q))
        if code == nat.NPP_ERR_INVALID:
            raise ValueError(self.lib.npp_last_error(self.h).decode())
        nat.check(self.h, code)
        n_base = self._goal["n_base"] if getattr(self, "_goal", None) else self.n_levels
        self._archive_meta = self._archive_cells = self._archive_route_views = None
        self._episode_views = None
        self._reward_mode, self._reward_pending = 0, False
        self._reward_waypoints = False
        self._pool_weights = None
        self._goal = None
        self._sweep = None
        self.n_levels = self.lib.npp_num_levels(self.h)
        if not on:
            return
        base_of, stage_of = np.zeros(self.n_levels, dtype=np.int32), np.zeros(self.n_levels, dtype=np.int32)
        nb = C.c_int()
        nat.check(self.h, self.lib.npp_goal_tables(self.h, base_of.ctypes.data_as(C.c_void_p), stage_of.ctypes.data_as(C.c_void_p), C.byref(nb)))
        assert nb.value == n_base
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        rw, need = C.c_int(), C.c_int()
        nat.check(self.h, self.lib.npp_goal_view(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(nb), C.byref(rw), C.byref(need)))
        lv = _device_tensor(a.value, len(self.GOAL_LEVEL_WORDS) * n_base, torch.int32, self.device).view(-1, n_base)
        env = _device_tensor(c.value, len(self.GOAL_ENV_WORDS) * self.n, torch.int32, self.device).view(-1, self.n)
        ring = _device_tensor(b.value, n_base * rw.value, torch.int32, self.device).view(n_base, rw.value)
        self._goal = {"n_base": n_base, "base_of": base_of, "stage_of": stage_of, "level_words": lv, "env_words": env, "ring": ring,
                      "need": need.value, "window": int(rolling_window), "interval": float(stage_distance_interval),
                      "auto_advance": bool(auto_advance)}

    def goal_set_stage(self, stage, level=None):
        """Deferred as in the reference: the stage takes effect at every env's next episode start; clamped to the last stage."""
        nat.check(self.h, self.lib.npp_goal_set_stage(self.h, -1 if level is None else int(level), int(stage)))

    def goal_views(self):
        """The mode's tables and device views (no copy): n_base, base_of / stage_of (numpy int32 [n_levels]), level_words int32
        [10, n_base] (rows GOAL_LEVEL_WORDS), env_words int32 [5, N] (rows GOAL_ENV_WORDS), ring int32 [n_base, words], need, window."""
        if getattr(self, "_goal", None) is None:
            raise ValueError("the goal curriculum is off (set_goal_curriculum)")
        return self._goal

    def goal_stage_positions(self, level):
        """-> (num_stages, distances f64[3], original f64[4], positions f64[max(num_stages, 1), 4]) of a base level"""
        ns = C.c_int32()
        dist, orig, pos = np.zeros(3), np.zeros(4), np.zeros((1024, 4))
        nat.check(self.h, self.lib.npp_goal_stage_positions(self.h, int(level), C.byref(ns), dist.ctypes.data_as(C.c_void_p),
                                                           orig.ctypes.data_as(C.c_void_p), 1024, pos.ctypes.data_as(C.c_void_p)))
        return ns.value, dist, orig, pos[:max(ns.value, 1)].copy()

    def assign_levels(self, level_ids, env_ids=None):
        lv = np.ascontiguousarray(level_ids, dtype=np.int32)
        if env_ids is None:
            nat.check(self.h, self.lib.npp_assign_levels(self.h, None, lv.ctypes.data_as(C.POINTER(C.c_int32)), len(lv)))
        else:
            ev = np.ascontiguousarray(env_ids, dtype=np.int32)
            nat.check(self.h, self.lib.npp_assign_levels(
                self.h, ev.ctypes.data_as(C.POINTER(C.c_int32)), lv.ctypes.data_as(C.POINTER(C.c_int32)), len(lv)))

    def set_truncation_limit(self, limit):
        if np.isscalar(limit):
            nat.check(self.h, self.lib.npp_set_truncation_limit(self.h, None, int(limit)))
        else:
            lim = np.ascontiguousarray(limit, dtype=np.int32)
            assert len(lim) == self.n
            nat.check(self.h, self.lib.npp_set_truncation_limit(self.h, lim.ctypes.data_as(C.POINTER(C.c_int32)), 0))

    def set_dynamic_truncation(self, enable=True):
        """The reference env's per-level limit: int(clip(sqrt(reachable surface area) * 500, 1200, 10000)) frames
        (truncation_calculator.py:19-57), re-applied at every level (re)assignment."""
        nat.check(self.h, self.lib.npp_set_dynamic_truncation(self.h, 1 if enable else 0))

    # ---- level pool (include/npp_amd.h npp_set_level_pool; the reference's per-episode map draw) -------------------
    def set_level_pool(self, weights, seed=0):
        """Draw a new level for every episode: level l with probability weights[l] / sum(weights) (one non-negative weight per
        loaded level).  weights=None turns the pool off.  A call with the pool's current seed keeps the per-env draw counts (a
        curriculum update); another seed restarts them.  Bad weights raise ValueError with the native message."""
        if weights is None:
            nat.check(self.h, self.lib.npp_set_level_pool(self.h, None, 0, 0))
            self._pool_weights = None
            return
        w = np.array(weights, dtype=np.float64).ravel()
        code = self.lib.npp_set_level_pool(self.h, w.ctypes.data_as(C.POINTER(C.c_double)), len(w), int(seed) & (2**64 - 1))
        if code == nat.NPP_ERR_INVALID:
            raise ValueError(self.lib.npp_last_error(self.h).decode())
        nat.check(self.h, code)
        self._pool_weights = w

    def draw_levels(self, mask=None):
        """Every env (or those with a non-zero mask byte) draws a level from the pool now; an env that draws another level is
        assigned it as by assign_levels (reset on it), the others are left alone."""
        if mask is None:
            nat.check(self.h, self.lib.npp_draw_levels(self.h, None))
        else:
            m = np.ascontiguousarray(mask, dtype=np.uint8)
            assert len(m) == self.n
            nat.check(self.h, self.lib.npp_draw_levels(self.h, m.ctypes.data_as(C.POINTER(C.c_uint8))))

    def env_level_view(self):
        """int32 CUDA tensor [N] over the handle's env -> level array (no copy): the draws rewrite it in stream order."""
        if getattr(self, "_level_view", None) is None:
            p = C.c_void_p()
            nat.check(self.h, self.lib.npp_env_level_view(self.h, C.byref(p)))
            self._level_view = _device_tensor(p.value, self.n, torch.int32, self.device)
        return self._level_view

    def env_levels(self):
        """int32 [N]: the level every env plays now (synchronises the handle's stream)."""
        out = np.zeros(self.n, dtype=np.int32)
        nat.check(self.h, self.lib.npp_get_env_levels(self.h, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def set_launch_geometry(self, lanes_per_env=0, waves_per_block=0):
        nat.check(self.h, self.lib.npp_set_launch_geometry(self.h, int(lanes_per_env), int(waves_per_block)))

    def set_step_variant(self, variant=-1):
        """Build variant of the step kernel: -1 = autotune on this handle's workload (default), 0..2 pin one (same bits either way)."""
        nat.check(self.h, self.lib.npp_set_step_variant(self.h, int(variant)))

    def set_obs_overlap(self, cuts=0):
        """Observation overlap (include/npp_amd.h npp_set_obs_overlap_parts): cut the step's heavy-first workgroup order at `cuts`
        (one percentage or up to three ascending ones) and run the pieces, and the observation kernels behind each, on streams of
        their own; 0 / () switches it off.  Same bits; call join() (to_host() does) before consuming the outputs."""
        cuts = [int(cuts)] if np.isscalar(cuts) else [int(c) for c in cuts]
        cuts = [c for c in cuts if c > 0]
        arr = (C.c_int * max(1, len(cuts)))(*cuts)
        nat.check(self.h, self.lib.npp_set_obs_overlap_parts(self.h, arr, len(cuts)))

    def join(self):
        nat.check(self.h, self.lib.npp_join(self.h))

    def step_variant(self):
        """(variant npp_step launches now, True once the autotuner has decided or a variant is pinned)"""
        v, t = C.c_int(0), C.c_int(0)
        nat.check(self.h, self.lib.npp_get_step_variant(self.h, C.byref(v), C.byref(t)))
        return v.value, bool(t.value)

    def launch_geometry(self):
        g, w = C.c_int(0), C.c_int(0)
        nat.check(self.h, self.lib.npp_get_launch_geometry(self.h, C.byref(g), C.byref(w)))
        return g.value, w.value

    # ---- stepping ---------------------------------------------------------------------------------------------
    def reset(self, mask=None, mode="default"):
        """mode: "default" (the handle's NPP_FLAG_FAST_RESET decides), "full" (Simulator.reset), "fast" (fast_reset)."""
        code = {"default": 0, "full": 1, "fast": 2}[mode]
        if mask is None:
            nat.check(self.h, self.lib.npp_reset_ex(self.h, None, code))
        else:
            m = np.ascontiguousarray(mask, dtype=np.uint8)
            assert len(m) == self.n
            nat.check(self.h, self.lib.npp_reset_ex(self.h, m.ctypes.data_as(C.POINTER(C.c_uint8)), code))

    def step(self, actions, frame_skip=4, want_terminal=True, work_out=None):
        """actions: uint8 CUDA tensor [N] with values 0..5.  Asynchronous; outputs land in self.game_state etc.
        work_out: optional int16 CUDA tensor [N] that receives this step's per-env depenetration iteration counts (instead
        of the block's `work` field) -- lets a profiler keep one row per step."""
        assert actions.dtype == torch.uint8 and actions.is_cuda and actions.numel() == self.n
        out = self._out if want_terminal else self._out_min
        if work_out is not None:
            assert work_out.dtype == torch.int16 and work_out.is_cuda and work_out.numel() == self.n and work_out.is_contiguous()
            tmp = nat.StepOut()
            C.memmove(C.byref(tmp), C.byref(out), C.sizeof(nat.StepOut))
            tmp.d_work = work_out.data_ptr()
            out = tmp
        nat.check(self.h, self.lib.npp_step(self.h, C.c_void_p(actions.data_ptr()), int(frame_skip), C.byref(out)))
        self._reward_pending = bool(self._reward_mode)

    def step_many(self, actions, frame_skip=4):
        """actions: uint8 CUDA tensor [K, N].  K Gymnasium steps in one launch (open-loop sequences: checkpoint replay, fixed
        plans).  Returns (flags u8 [K, N], reward f32 [K, N], frames i16 [K, N]); observations of the last step land in
        self.game_state etc.; with auto-reset, envs that terminate mid-sequence restart on the spot.  Nothing is pushed onto
        the frame stacks (NppVecEnvironment re-pads them from the observation after a checkpoint replay).
        Raises ValueError while action masking is on (set_action_masking): its counters need every observation; likewise while
        reward mode "pbrs" is on (set_reward_mode): the reward needs the observation of every step."""
        assert actions.dtype == torch.uint8 and actions.is_cuda and actions.dim() == 2 and actions.shape[1] == self.n
        if self._reward_mode:
            raise ValueError('step_many with reward mode "pbrs" on: the reward is computed once per observation and the launch\'s '
                             'inner steps have none (set_reward_mode("sparse") first)')
        if self._masking:
            raise ValueError("step_many with action masking on: the detector runs once per observation and the launch's inner "
                             "steps have none (set_action_masking(0) first)")
        K = int(actions.shape[0])
        with self._ctx():   # allocations, the launch and the copies below are all ordered on the handle's stream
            actions = actions.contiguous()
            flags = torch.zeros((K, self.n), dtype=torch.uint8, device=self.device)
            reward = torch.zeros((K, self.n), dtype=torch.float32, device=self.device)
            frames = torch.zeros((K, self.n), dtype=torch.int16, device=self.device)
            out = nat.StepOut(self.game_state.data_ptr(), self.action_mask.data_ptr(), self.entity_pos.data_ptr(), flags.data_ptr(),
                              reward.data_ptr(), frames.data_ptr(), None,
                              self.spatial_context.data_ptr() if self.spatial_context is not None else None,
                              self.positions.data_ptr() if self.positions is not None else None, None)
            nat.check(self.h, self.lib.npp_step_many(self.h, C.c_void_p(actions.data_ptr()), K, int(frame_skip), C.byref(out)))
            self._keep = actions
            self.flags.copy_(flags[-1]); self.reward.copy_(reward[-1]); self.frames.copy_(frames[-1])
        return flags, reward, frames

    def tick(self, inputs):
        """inputs: uint8 CUDA tensor [T, N] of replay input bytes (bit0 jump, bit1 right, bit2 left)."""
        assert inputs.dtype == torch.uint8 and inputs.is_cuda and inputs.dim() == 2 and inputs.shape[1] == self.n
        inputs = inputs.contiguous()
        nat.check(self.h, self.lib.npp_tick(self.h, C.c_void_p(inputs.data_ptr()), int(inputs.shape[0])))
        self._keep = inputs

    def observe(self, flags_out=None):
        """Write the observation of the current state into the block.  flags_out: uint8 CUDA tensor [N] that receives the
        flags of the observed state instead of the block; the block's flags, reward, frames and work then keep describing the
        last step (NppVecEnvironment.restart observes between two steps)."""
        if flags_out is None:
            nat.check(self.h, self.lib.npp_observe(self.h, C.byref(self._out_min)))
            return
        assert flags_out.dtype == torch.uint8 and flags_out.is_cuda and flags_out.numel() == self.n and flags_out.is_contiguous()
        out = nat.StepOut()
        C.memmove(C.byref(out), C.byref(self._out_min), C.sizeof(nat.StepOut))
        out.d_flags, out.d_reward, out.d_frames, out.d_work = flags_out.data_ptr(), None, None, None
        nat.check(self.h, self.lib.npp_observe(self.h, C.byref(out)))

    def render_player_frame(self, out=None):
        """out: uint8 CUDA tensor [N, 84, 84] (or [N, 84, 84, 1]) filled with the player_frame of every env; default: the
        output block's player_frame field (enable_outputs("player_frame"))."""
        if out is None:
            out = self.out.t["player_frame"]
        assert out.dtype == torch.uint8 and out.is_cuda and out.numel() == self.n * 84 * 84 and out.is_contiguous()
        nat.check(self.h, self.lib.npp_render_player_frame(self.h, C.c_void_p(out.data_ptr())))

    def set_entity_pos(self, env, kind, x, y):
        """Move the exit switch (kind 0) or exit door (kind 1) of one env (curriculum repositioning); NaN clears."""
        nat.check(self.h, self.lib.npp_set_entity_pos(self.h, int(env), int(kind), float(x), float(y)))

    def switch_states(self, out=None):
        """float32 CUDA tensor [N, 25]: the reference's switch_states observation (5 locked doors x 5 features)."""
        if out is None:
            out = self.out.t.get("switch_states")
        if out is None:
            with self._ctx():
                out = torch.zeros((self.n, 25), dtype=torch.float32, device=self.device)
        assert out.dtype == torch.float32 and out.is_cuda and out.numel() == self.n * 25 and out.is_contiguous()
        nat.check(self.h, self.lib.npp_switch_states(self.h, C.c_void_p(out.data_ptr())))
        return out

    def reachability(self, with_switch_states=False):
        """Fill the block's reachability_features [N, 38] / mine_sdf_features [N, 3] / reach_status [N] (whichever are
        enabled) from the current state.  Call once per observation: the 38 floats follow the reference's cache rule
        (recomputed when the ninja's 24-px cell or exit_switch_activated changed since the previous call).
        with_switch_states: also fill the block's switch_states from the same launch (instead of a switch_states() call)."""
        t = self.out.t
        ptr = [C.c_void_p(t[k].data_ptr()) if k in t else None for k in ("reachability_features", "mine_sdf_features", "reach_status")]
        if ptr[0] is None and ptr[1] is None:
            raise RuntimeError('enable_outputs("reachability_features") and / or "mine_sdf_features" first')
        sw = C.c_void_p(t["switch_states"].data_ptr()) if with_switch_states else None
        nat.check(self.h, self.lib.npp_reachability_ex(self.h, *ptr, sw))

    def minimal_observation(self, out=None):
        """float32 CUDA tensor [N, 40]: the reference's minimal observation (compute_minimal_observation) of the current state;
        default: the block's minimal_observation field (outputs=("minimal_observation",) / enable_outputs).  It is this
        observation's reachability call (same cache rule; fills reach_status when enabled) -- call it once per observation, after
        step() / observe(), instead of or beside reachability()."""
        t = self.out.t
        if "minimal_observation" not in t:
            raise RuntimeError('enable_outputs("minimal_observation") first: it switches the mode on for the step launches')
        if out is None:
            out = t["minimal_observation"]
        assert out.dtype == torch.float32 and out.is_cuda and out.numel() == self.n * 40 and out.is_contiguous()
        st = C.c_void_p(t["reach_status"].data_ptr()) if "reach_status" in t else None
        nat.check(self.h, self.lib.npp_minimal_observation(self.h, C.c_void_p(out.data_ptr()), st))
        return out

    # ---- reward mode "pbrs" (include/npp_amd.h npp_set_reward_mode) ------------------------------------
    REWARD_MODES = {None: 0, "sparse": 0, "pbrs": 1, 0: 0, 1: 1}

    def _reward_params_struct(self, params):
        """None, a dict with some of REWARD_PARAMS (the others keep the reference's defaults) or a sequence of all six -> the six
        doubles of NppRewardParams"""
        q = (C.c_double * 6)()
        self.lib.npp_reward_default_params(q)
        if params is None:
            return q
        if isinstance(params, dict):
            for k, v in params.items():
                if k not in REWARD_PARAMS:
                    raise ValueError("unknown reward parameter %r (parameters: %s)" % (k, ", ".join(REWARD_PARAMS)))
                q[REWARD_PARAMS.index(k)] = float(v)
            return q
        if len(params) != 6:
            raise ValueError("reward parameters: a dict or the six values %s" % (REWARD_PARAMS,))
        for i, v in enumerate(params):
            q[i] = float(v)
        return q

    def set_reward_mode(self, mode, params=None):
        """"sparse" (default): the block's reward holds the step kernel's three constants.  "pbrs": step_reward() after every step()
        overwrites it with the reference's RewardCalculator.calculate_reward (potential-based shaping on path distance, milestones,
        terminal rewards).  Switching "pbrs" on restarts every env's reward state on its current state.  Raises
        NppError (NPP_ERR_UNSUPPORTED) for a level set the reference's reward cannot handle; the mode then stays off."""
        if mode not in self.REWARD_MODES:
            raise ValueError('reward mode must be "sparse" or "pbrs", not %r' % (mode,))
        code = self.REWARD_MODES[mode]
        self._reward_mode = 0
        self._reward_pending = False
        if not code:
            self._reward_waypoints = False   # (the path waypoints go with the mode)
        nat.check(self.h, self.lib.npp_set_reward_mode(self.h, code, self._reward_params_struct(params) if code else None))
        self._reward_mode = code

    def set_reward_params(self, params=None):
        """New RewardConfig numbers (REWARD_PARAMS) from the next step_reward() on; None: the reference's defaults."""
        nat.check(self.h, self.lib.npp_set_reward_params(self.h, self._reward_params_struct(params)))

    def _waypoint_params_struct(self, params):
        """None, a dict with some of WAYPOINT_PARAMS (the others keep the reference's defaults) or a sequence of all four -> the four
        doubles of NppWaypointParams"""
        q = (C.c_double * 4)()
        self.lib.npp_waypoint_default_params(q)
        if params is None:
            return q
        if isinstance(params, dict):
            for k, v in params.items():
                if k not in WAYPOINT_PARAMS:
                    raise ValueError("unknown waypoint parameter %r (parameters: %s)" % (k, ", ".join(WAYPOINT_PARAMS)))
                q[WAYPOINT_PARAMS.index(k)] = float(v)
            return q
        if len(params) != 4:
            raise ValueError("waypoint parameters: a dict or the four values %s" % (WAYPOINT_PARAMS,))
        for i, v in enumerate(params):
            q[i] = float(v)
        return q

    def set_reward_waypoints(self, on, params=None):
        """Reward mode "pbrs" only: the sequential path waypoints of a fresh RewardConfig().  On: every loaded level's
        waypoint table is built (progress_spacing takes effect here only) and step_reward() adds the bonus of collecting the next
        waypoint along the optimal path; every env's collection state restarts.  Raises NppError: NPP_ERR_STATE with the mode off,
        NPP_ERR_UNSUPPORTED for a level with more than 512 waypoints, NPP_ERR_INVALID for a collection radius above 24."""
        self._reward_waypoints = False
        nat.check(self.h, self.lib.npp_set_reward_waypoints(self.h, 1 if on else 0, self._waypoint_params_struct(params) if on else None))
        self._reward_waypoints = bool(on)

    def set_waypoint_params(self, params=None):
        """New collection radius and scales (WAYPOINT_PARAMS; progress_spacing is ignored) from the next step_reward() on; None: the
        reference's defaults."""
        nat.check(self.h, self.lib.npp_set_waypoint_params(self.h, self._waypoint_params_struct(params)))

    def level_waypoints(self, level):
        """(xy f64 [count, 2] world pixels, phase u8 [count]: 0 pre-switch, 1 post-switch) of a loaded level, in sequence order."""
        count = C.c_int32(0)
        nat.check(self.h, self.lib.npp_reward_waypoints(self.h, int(level), None, None, 0, C.byref(count)))
        xy, ph = np.zeros((count.value, 2), dtype=np.float64), np.zeros(count.value, dtype=np.uint8)
        nat.check(self.h, self.lib.npp_reward_waypoints(self.h, int(level), xy.ctypes.data_as(C.c_void_p), ph.ctypes.data_as(C.c_void_p),
                                                        count.value, C.byref(count)))
        return xy, ph

    def step_reward(self, status_out=None, wp_bonus_out=None, wp_info_out=None):
        """One call per step(), after it: the reference's step reward of every env into the block's reward, and its unscaled
        components (REWARD_COMPONENTS) into reward_components when that output is enabled.  status_out: optional int32 CUDA tensor
        [N]: 0 the potential was evaluated in full, 1 from the position cache, 2 from it without next hop, 3 not at all (terminal
        step).  With the path waypoints on: wp_bonus_out (optional float32 CUDA tensor [N]) the step's UNSCALED waypoint bonus,
        wp_info_out (optional int32 CUDA tensor [N, 3]) the collected sequence index or -1, the next expected index, the collected
        count; with them off neither is written.  Enqueued on the handle's stream, so to_host() after it stages the new reward."""
        if not self._reward_mode:
            raise ValueError('step_reward: reward mode "pbrs" is off (set_reward_mode("pbrs"))')
        if not self._reward_pending:
            raise ValueError("step_reward: no step() since the last call, or the output block was re-allocated since (one call per step)")
        t = self.out.t
        comp = C.c_void_p(t["reward_components"].data_ptr()) if "reward_components" in t else None
        st = None
        if status_out is not None:
            assert status_out.dtype == torch.int32 and status_out.is_cuda and status_out.numel() == self.n and status_out.is_contiguous()
            st = C.c_void_p(status_out.data_ptr())
        wb = wi = None
        if wp_bonus_out is not None:
            assert wp_bonus_out.dtype == torch.float32 and wp_bonus_out.is_cuda and wp_bonus_out.numel() == self.n and wp_bonus_out.is_contiguous()
            wb = C.c_void_p(wp_bonus_out.data_ptr())
        if wp_info_out is not None:
            assert wp_info_out.dtype == torch.int32 and wp_info_out.is_cuda and wp_info_out.numel() == self.n * 3 and wp_info_out.is_contiguous()
            wi = C.c_void_p(wp_info_out.data_ptr())
        nat.check(self.h, self.lib.npp_step_reward_wp(self.h, C.c_void_p(self.reward.data_ptr()), comp, st, wb, wi))
        self._reward_pending = False

    # ---- path-direction action masking (include/npp_amd.h npp_set_action_masking) ---------------------
    MASKING_MODES = {None: 0, "none": 0, "off": 0, "hard": 1, "soft": 2, 0: 0, 1: 1, 2: 2}

    def set_action_masking(self, mode):
        """The reference env's action-masking mode (reward_config.py:815-865): "hard" -- path_action_mask() filters the block's
        action_mask by the straight-path direction, "soft" -- it writes the direction only, None / "none" -- off (default: nothing
        is launched).  May change between any two steps."""
        if mode not in self.MASKING_MODES:
            raise ValueError('action masking mode must be None, "none", "hard" or "soft", not %r' % (mode,))
        self._masking = self.MASKING_MODES[mode]
        nat.check(self.h, self.lib.npp_set_action_masking(self.h, self._masking))

    def path_action_mask(self, status_out=None):
        """One call per observation, after step() / observe() / reset(): the reference's _detect_straight_path_direction for every
        env, into the block's path_direction (i8 [N]: 0 none, 1 left, 2 right, 3 down; enable_outputs("path_direction")), and in
        hard mode its mask stage applied to the block's action_mask in place.  status_out: optional int32 CUDA tensor [N], 1 where
        the direction came from the graph.  Enqueued on the handle's stream, so to_host() after it stages the filtered mask."""
        t = self.out.t
        d = C.c_void_p(t["path_direction"].data_ptr()) if "path_direction" in t else None
        st = None
        if status_out is not None:
            assert status_out.dtype == torch.int32 and status_out.is_cuda and status_out.numel() == self.n and status_out.is_contiguous()
            st = C.c_void_p(status_out.data_ptr())
        nat.check(self.h, self.lib.npp_path_action_mask(self.h, C.c_void_p(self.action_mask.data_ptr()), d, st))

    def path_mask_stats(self):
        """{"observed", "applied", "last_observed", "last_applied"}: int32 CUDA views [N] of the handle's counters (no copy; the
        device holds them as u32) -- detector calls since the env's last reset, those classified from the graph, and both as
        latched when the env's last episode ended in an auto-reset.  They count calls of path_action_mask(): a second call for the
        same state counts again.  reset() and switching the mode from off to on restart the live ones.  Not part of archive /
        snapshot records."""
        if self._mask_stats is None:
            p = [C.c_void_p() for _ in range(4)]
            nat.check(self.h, self.lib.npp_path_mask_stats_view(self.h, *[C.byref(x) for x in p]))
            self._mask_stats = {k: _device_tensor(x.value, self.n, torch.int32, self.device)
                                for k, x in zip(("observed", "applied", "last_observed", "last_applied"), p)}
        return self._mask_stats

    def graph_observation(self, node_feats=None, edge_index=None, node_mask=None, edge_mask=None, rewrite_all=False):
        """The graph observations of every env (include/npp_amd.h npp_graph_observation): graph_node_feats f32 [N, 2500, 6],
        graph_edge_index u16 [N, 2, 20000], graph_node_mask u8 [N, 2500], graph_edge_mask u8 [N, 20000], CUDA tensors updated
        in place.  They are a constant of each env's level: only the rows of envs whose level changed since the last call are
        rewritten.  Without arguments the four tensors are the batch's own (allocated at the first call, 162.5 KB per env,
        outside the packed output block); a call with other tensors, or rewrite_all, rewrites every row.  Returns the four
        tensors as a dict keyed by observation name."""
        given = (node_feats, edge_index, node_mask, edge_mask)
        if all(t is None for t in given):
            if getattr(self, "_graph", None) is None:
                with self._ctx():
                    # (zeroed as int16: uint16 tensors have few kernels; the native call writes every row anyway)
                    self._graph = {k: torch.zeros((self.n,) + shape, dtype=torch.int16 if dt == torch.uint16 else dt,
                                                  device=self.device).view(dt) for k, (shape, dt) in GRAPH_KEYS.items()}
            bufs = self._graph
        else:
            bufs = dict(zip(GRAPH_KEYS, given))
            for k, (shape, dt) in GRAPH_KEYS.items():
                t = bufs[k]
                assert t is not None and t.dtype == dt and t.is_cuda and t.is_contiguous() and tuple(t.shape) == (self.n,) + shape, k
        nat.check(self.h, self.lib.npp_graph_observation(self.h, *[C.c_void_p(bufs[k].data_ptr()) for k in GRAPH_KEYS],
                                                         1 if rewrite_all else 0))
        return bufs

    def render_frame(self, env0=0, count=1):
        """uint8 CUDA tensor [count, 600, 1056, 1]: the whole gray frame (the reference's render() array) of some envs."""
        with self._ctx():
            out = torch.zeros((count, 600, 1056, 1), dtype=torch.uint8, device=self.device)
        nat.check(self.h, self.lib.npp_render_frame(self.h, int(env0), int(count), C.c_void_p(out.data_ptr())))
        return out

    def render_global_view(self, out=None):
        """out: uint8 CUDA tensor [N, 176, 100] (or [N, 176, 100, 1]): the reference's global_view of every env."""
        if out is None:
            out = self.out.t["global_view"]
        assert out.dtype == torch.uint8 and out.is_cuda and out.numel() == self.n * 176 * 100 and out.is_contiguous()
        nat.check(self.h, self.lib.npp_render_global_view(self.h, C.c_void_p(out.data_ptr())))

    def entity_checksum(self, env0=0, count=None):
        """[count, 6] f64: per-env sums over all entities in entity_dic order (see npp_entity_checksum)."""
        count = self.n - env0 if count is None else count
        o = np.zeros((count, 6), dtype=np.float64)
        nat.check(self.h, self.lib.npp_entity_checksum(self.h, env0, count, o.ctypes.data_as(C.POINTER(C.c_double))))
        return o

    def snapshot(self):
        """Checkpoint the state of every env on the device (one slot)."""
        nat.check(self.h, self.lib.npp_snapshot(self.h))

    def restore(self, mask=None):
        """Put the checkpointed state back (for the masked envs; None = all)."""
        if mask is None:
            nat.check(self.h, self.lib.npp_restore(self.h, None))
        else:
            m = np.ascontiguousarray(mask, dtype=np.uint8)
            assert len(m) == self.n
            nat.check(self.h, self.lib.npp_restore(self.h, m.ctypes.data_as(C.POINTER(C.c_uint8))))

    # ---- checkpoint archive (include/npp_amd.h npp_archive_create; the reference's Go-Explore checkpoints) ----------
    def archive_create(self, n_slots):
        """Allocate the checkpoint archive: n_slots records of one env's state each (0 frees it).  Needs levels loaded;
        load_levels drops it."""
        n_slots = int(n_slots)
        if n_slots < 0:
            raise ValueError("archive_create: n_slots must be >= 0 (0 frees the archive)")
        nat.check(self.h, self.lib.npp_archive_create(self.h, n_slots))
        self._archive_meta = self._archive_cells = self._archive_route_views = None

    def archive_num_slots(self):
        return int(self.lib.npp_archive_num_slots(self.h))

    def archive_record_bytes(self):
        """Size of one slot's record in bytes (follows from the loaded level set); 0 without an archive."""
        return int(self.lib.npp_archive_record_bytes(self.h))

    def _archive_lists(self, envs, slots, unique, what):
        """The two lists as int32 CUDA tensors of one length (check_archive_lists, then arrays are uploaded)."""
        lists = check_archive_lists(envs, slots, unique, what)
        out = []
        with self._ctx():
            for name in ("envs", "slots"):
                v = lists[name]
                if isinstance(v, np.ndarray):
                    v = torch.from_numpy(np.ascontiguousarray(v, dtype=np.int32)).to(self.device)
                elif not v.is_cuda:
                    v = v.to(self.device)
                out.append(v.contiguous())
        return out

    def _archive_move(self, fn, envs, slots, status, unique, what):
        e, s = self._archive_lists(envs, slots, unique, what)
        st = None
        if status:
            with self._ctx():
                st = torch.empty(len(e), dtype=torch.int32, device=self.device)
        nat.check(self.h, fn(self.h, C.c_void_p(e.data_ptr()), C.c_void_p(s.data_ptr()), len(e),
                             C.c_void_p(st.data_ptr()) if st is not None else None))
        self._keep_archive = (e, s)   # the launch reads the lists in stream order
        return st

    def archive_store(self, envs, slots, status=False):
        """Entry i copies the state of env envs[i] into slot slots[i].  envs / slots: int32 CUDA tensors [count] (used where
        they are, nothing synchronises), or integer arrays (uploaded; a slot that comes twice raises ValueError).  A negative
        env or slot skips the entry.  status=True returns the device status tensor i32 [count]: 0 done, 1 skipped, 4 out of
        range."""
        return self._archive_move(self.lib.npp_archive_store, envs, slots, status, "slots", "archive_store")

    def archive_restore(self, envs, slots, status=False):
        """Entry i puts the record of slot slots[i] into env envs[i] (any env playing the record's level; one slot may go to
        many envs).  Arguments as archive_store (an env that comes twice in an array raises ValueError).  Status: 0 done,
        1 skipped, 2 the slot's level is not the env's, 3 the slot is empty, 4 out of range -- only status 0 touches the env."""
        return self._archive_move(self.lib.npp_archive_restore, envs, slots, status, "envs", "archive_restore")

    def archive_meta(self):
        """{"x", "y", "vx", "vy": f64 [n_slots]; "stored", "level", "frame", "cell_x", "cell_y", "switch_activated": i32
        [n_slots]}: CUDA views (no copy) of the rows the store kernel writes, valid while the archive lives."""
        if getattr(self, "_archive_meta", None) is None:
            f, i = C.c_void_p(), C.c_void_p()
            nat.check(self.h, self.lib.npp_archive_meta_view(self.h, C.byref(f), C.byref(i)))
            ns = self.archive_num_slots()
            tf = _device_tensor(f.value, ns * 4, torch.float64, self.device).view(ns, 4)
            ti = _device_tensor(i.value, ns * 6, torch.int32, self.device).view(ns, 6)
            meta = {k: tf[:, c] for c, k in enumerate(("x", "y", "vx", "vy"))}
            meta.update({k: ti[:, c] for c, k in enumerate(("stored", "level", "frame", "cell_x", "cell_y", "switch_activated"))})
            self._archive_meta = meta
        return self._archive_meta

    # ---- action routes (include/npp_amd.h npp_set_routes; the reference's _action_sequence) ---------------
    def set_routes(self, capacity):
        """Record every env's action route on the device: `capacity` actions per route (rounded up to a multiple of 16; 0
        switches it off and frees the buffers).  Before archive_create: the archive's records then carry each slot's route.
        Invalidates the snapshot."""
        capacity = int(capacity)
        if capacity < 0:
            raise ValueError("set_routes: capacity must be >= 0 (0 switches the routes off)")
        nat.check(self.h, self.lib.npp_set_routes(self.h, capacity))
        self._route_views = self._archive_route_views = None

    def route_views(self):
        """(actions u8 [N, 2, cap], header i32 [N, 16]): CUDA views (no copy) of the handle's route buffers and headers,
        rewritten in stream order.  Header words 0-5 describe the current route (len, bits, frame_skip, frames, last flags, level),
        6-11 the finished one, word 12 says which of the two buffers holds the current route."""
        if getattr(self, "_route_views", None) is None:
            a, hd, cap = C.c_void_p(), C.c_void_p(), C.c_int(0)
            nat.check(self.h, self.lib.npp_route_view(self.h, C.byref(a), C.byref(hd), C.byref(cap)))
            self._route_views = (_device_tensor(a.value, self.n * 2 * cap.value, torch.uint8, self.device).view(self.n, 2, cap.value),
                                 _device_tensor(hd.value, self.n * 16, torch.int32, self.device).view(self.n, 16))
        return self._route_views

    def archive_route_views(self):
        """(actions u8 [n_slots, cap], header i32 [n_slots, 8]): strided CUDA views (no copy) over the archive's records of
        each slot's route -- header words as in route_views (0-5; 6-7 are 0)."""
        if getattr(self, "_archive_route_views", None) is None:
            rec, off, stride = C.c_void_p(), C.c_int64(), C.c_int64()
            nat.check(self.h, self.lib.npp_archive_route_view(self.h, C.byref(rec), C.byref(off), C.byref(stride)))
            ns, off, stride = self.archive_num_slots(), off.value, stride.value
            cap = self.archive_record_bytes() - (off + 8) * 4
            words = _device_tensor(rec.value, ns * stride, torch.int32, self.device)
            raw = _device_tensor(rec.value, ns * stride * 4, torch.uint8, self.device)
            self._archive_route_views = (torch.as_strided(raw, (ns, cap), (stride * 4, 1), (off + 8) * 4),
                                         torch.as_strided(words, (ns, 8), (stride, 1), off))
        return self._archive_route_views

    # ---- episode statistics (include/npp_amd.h npp_set_episode_stats) ------------------------------------
    EPISODE_COLUMNS = ("episodes", "won", "dead", "truncated", "dead_mine", "dead_impact", "switch", "steps", "frames", "won_frames",
                       "return_fix", "restored", "abandoned")
    _EPISODE_I32 = ("steps", "frames", "switch_step", "switch_frames", "level", "bits")

    def set_episode_stats(self, on=True):
        """Keep per-env episode records (return, length, switch latch, level) and a per-level outcome table on the device; off
        frees them.  After load_levels: the table has a row per loaded level, and load_levels switches the feature off."""
        nat.check(self.h, self.lib.npp_set_episode_stats(self.h, 1 if on else 0))
        self._episode_views = None

    def episode_accumulate(self, flags=None, frames=None, reward=None, components=None, n_steps=1, ended=None):
        """One call per step() / step_many(), after step_reward() when the reward comes from there: the rows' steps, frames and
        rewards go into the current episode of every env, and an ending row moves it to the finished one and into the level
        table.  flags u8 / frames i16 / reward f32 CUDA tensors of n_steps * N elements (default: the block's own, one row);
        components: f32 [n_steps * N, 6] or None; ended: optional u8 CUDA tensor [N], 1 where this call finished an episode."""
        flags = self.flags if flags is None else flags
        frames = self.frames if frames is None else frames
        reward = self.reward if reward is None else reward
        n_steps = int(n_steps)
        want = n_steps * self.n
        for name, t, dts, per in (("flags", flags, (torch.uint8,), 1), ("frames", frames, (torch.int16, torch.uint16), 1),
                                  ("reward", reward, (torch.float32,), 1), ("components", components, (torch.float32,), 6),
                                  ("ended", ended, (torch.uint8,), 0)):
            if t is None:
                continue
            if n_steps < 1 or t.dtype not in dts or not t.is_cuda or not t.is_contiguous() or t.numel() != (want * per if per else self.n):
                raise ValueError("episode_accumulate: %s must be a contiguous %s CUDA tensor of %s elements and n_steps >= 1"
                                 % (name, str(dts[0]).replace("torch.", ""), "N" if not per else "n_steps * N * %d" % per))
        nat.check(self.h, self.lib.npp_episode_accumulate(
            self.h, C.c_void_p(flags.data_ptr()), C.c_void_p(frames.data_ptr()), C.c_void_p(reward.data_ptr()),
            C.c_void_p(components.data_ptr()) if components is not None else None, n_steps,
            C.c_void_p(ended.data_ptr()) if ended is not None else None))
        self._keep_episode = (flags, frames, reward, components)

    def episode_restart(self, mask=None, from_restore=False):
        """The current episode of the envs under `mask` (u8 CUDA tensor [N], None = all) starts over: a running one counts as
        abandoned.  from_restore: the new episode does not start at the spawn -- it will add to `restored` only."""
        m = None
        if mask is not None:
            if mask.dtype != torch.uint8 or not mask.is_cuda or mask.numel() != self.n or not mask.is_contiguous():
                raise ValueError("episode_restart: mask must be a contiguous uint8 CUDA tensor [N]")
            m = C.c_void_p(mask.data_ptr())
            self._keep_episode_mask = mask
        nat.check(self.h, self.lib.npp_episode_restart(self.h, m, 1 if from_restore else 0))

    def episode_views(self):
        """Named CUDA views (no copy) of the records, rewritten in stream order: for the current episode steps, frames,
        switch_step, switch_frames, level, bits (int32 [N]), ret (float64 [N]) and comp (float64 [6, N]); the same with the
        prefix "fin_" for the finished one, plus fin_flags and n_finished; "table" int64 [L, 16]."""
        if getattr(self, "_episode_views", None) is None:
            a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
            nat.check(self.h, self.lib.npp_episode_view(self.h, C.byref(a), C.byref(b), C.byref(c)))
            i32 = _device_tensor(a.value, 14 * self.n, torch.int32, self.device).view(14, self.n)
            f64 = _device_tensor(b.value, 14 * self.n, torch.float64, self.device).view(14, self.n)
            v = {"i32": i32, "f64": f64,
                 "table": _device_tensor(c.value, self.n_levels * 16, torch.int64, self.device).view(self.n_levels, 16)}
            for k, name in enumerate(self._EPISODE_I32):
                v[name], v["fin_" + name] = i32[k], i32[6 + k]
            v["fin_flags"], v["n_finished"] = i32[12], i32[13]
            v["ret"], v["comp"], v["fin_ret"], v["fin_comp"] = f64[0], f64[1:7], f64[7], f64[8:14]
            self._episode_views = v
        return self._episode_views

    def episode_level_table(self):
        """int64 [L, 16] view of the level table (columns EPISODE_COLUMNS, then zeros); return_fix is the sum of the returns in
        units of 2^-20."""
        return self.episode_views()["table"]

    def episode_table_reset(self):
        nat.check(self.h, self.lib.npp_episode_table_reset(self.h))

    # ---- evaluation sweep (include/npp_amd.h npp_sweep_start) ---------------------------------------------
    _SWEEP_I32 = _EPISODE_I32 + ("flags", "env", "status")

    def sweep_start(self, jobs):
        """Play the level ids of `jobs` once each, in list order: env e starts on job e and every env takes the next job of the list
        when its episode ends (behind step(), in the place of the level pool's draw); an env that finds the list used up idles.
        Needs set_episode_stats(), and one episode_accumulate() behind every step().  A bad list raises ValueError."""
        j = np.ascontiguousarray(jobs, dtype=np.int32).ravel()
        if len(j) == 0:
            raise ValueError("sweep_start: the job list is empty")
        code = self.lib.npp_sweep_start(self.h, j.ctypes.data_as(C.c_void_p), len(j))
        if code == nat.NPP_ERR_INVALID:
            raise ValueError(self.lib.npp_last_error(self.h).decode())
        nat.check(self.h, code)
        a, b, c, d = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        nj = C.c_int()
        nat.check(self.h, self.lib.npp_sweep_view(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(nj)))
        J = nj.value
        i32 = _device_tensor(b.value, len(self._SWEEP_I32) * J, torch.int32, self.device).view(-1, J)
        f64 = _device_tensor(c.value, 7 * J, torch.float64, self.device).view(7, J)
        v = {"jobs": j.copy(), "n_jobs": J, "env_job": _device_tensor(a.value, self.n, torch.int32, self.device),
             "counters": _device_tensor(d.value, 3, torch.int32, self.device), "i32": i32, "f64": f64, "ret": f64[0], "comp": f64[1:7]}
        for k, name in enumerate(self._SWEEP_I32):
            v[name] = i32[k]
        self._sweep = v

    def sweep_stop(self):
        """End the sweep: every env keeps the level it plays.  The result views of sweep_state() stay readable."""
        nat.check(self.h, self.lib.npp_sweep_stop(self.h))

    def sweep_state(self):
        """Device views (no copy) of the last sweep started on this level set, rewritten in stream order: "jobs" (numpy int32 [J]),
        "n_jobs", "env_job" int32 [N] (-1 = idle), "counters" int32 [3] = next, done, n_jobs, and per job the result planes "i32"
        [9, J] (rows steps, frames, switch_step, switch_frames, level, bits, flags, env, status) and "f64" [7, J] (ret, comp)."""
        if getattr(self, "_sweep", None) is None:
            raise ValueError("no evaluation sweep was started on this level set (sweep_start)")
        return self._sweep

    # ---- cell index over the archive (include/npp_amd.h npp_archive_cells_create) ------------------------
    def archive_cells_create(self, seed=0, enable=True):
        """Go-Explore's cell index over the checkpoint archive: empties the archive and owns its slots from then on (archive_store
        is refused); archive_explore keeps the best state per (level, switch, 24 px cell), archive_select draws slots by visit
        count.  enable=False frees the tables and leaves the records.  Needs archive_create first."""
        nat.check(self.h, self.lib.npp_archive_cells_create(self.h, 1 if enable else 0, int(seed) & (2**64 - 1)))
        self._archive_cells = None

    def _cell_arg(self, v, dtype, what):
        """A per-env argument of the cell calls as a contiguous CUDA tensor [n] (a CUDA tensor is used where it is), or None."""
        if v is None:
            return None
        v = check_cell_arg(v, dtype, self.n, what)
        with self._ctx():
            if isinstance(v, np.ndarray):
                v = torch.from_numpy(v).to(self.device)
            elif not v.is_cuda:
                v = v.to(self.device)
            return v.contiguous()

    def archive_explore(self, score=None, mask=None, status=False):
        """Look at every env (mask: u8 / bool [n], None = all) and keep the best state per cell in slots the index allocates.
        score: f32 [n], larger is better; None = -(frame), the fewest frames to reach the cell.  CUDA tensors are used where
        they are, arrays are uploaded; nothing synchronises.  status=True returns the device tensor i32 [n]: 0 stored (won a new
        or a better cell), 1 skipped, 5 not eligible, 6 lost, 7 archive full."""
        sc = self._cell_arg(score, torch.float32, "archive_explore: score")
        m = self._cell_arg(mask, torch.uint8, "archive_explore: mask")
        st = None
        if status:
            with self._ctx():
                st = torch.empty(self.n, dtype=torch.int32, device=self.device)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
        nat.check(self.h, self.lib.npp_archive_explore(self.h, ptr(sc), ptr(m), ptr(st)))
        self._keep_archive = (sc, m)   # the launches read them in stream order
        return st

    SEED_SCORE_MODES = {"progress": 0, "frames": 1, "table": 2, 0: 0, 1: 1, 2: 2}

    def archive_seed(self, inputs, offsets, levels, score_mode, scores=None, counts=False):
        """Seed the cell index from recorded replays (include/npp_amd.h npp_archive_seed): replay r has the input
        bytes inputs[offsets[r]:offsets[r + 1]] (u8, i64 [R + 1] from 0) and is played on level levels[r] of the loaded set with this
        handle's envs as players; the state after every tick is offered to the index as by archive_explore, without counting
        visits.  score_mode: "progress" (tick / length, the reference seeder's score), "frames" (archive_explore's score=None) or
        "table" with scores: f32 [offsets[R]], ragged like the inputs (a CUDA tensor is used where it is; NaN = not eligible).
        counts=True returns the device tensor i32 [R, 4]: candidates, eligible, stored, archive full per replay.  Leaves the handle
        on the last round's levels with every route empty: assign_levels + reset afterwards.  Synchronises."""
        if score_mode not in self.SEED_SCORE_MODES:
            raise ValueError('archive_seed: score_mode must be "progress", "frames" or "table", not %r' % (score_mode,))
        mode = self.SEED_SCORE_MODES[score_mode]
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        lv = np.ascontiguousarray(levels, dtype=np.int32)
        if off.ndim != 1 or lv.ndim != 1 or len(off) != len(lv) + 1:
            raise ValueError("archive_seed: offsets must be [R + 1] for levels [R]")
        inp = np.ascontiguousarray(inputs, dtype=np.uint8).ravel()
        if len(off) and len(inp) < int(off[-1]):
            raise ValueError("archive_seed: inputs holds %d bytes, offsets[-1] is %d" % (len(inp), int(off[-1])))
        sc = None
        if mode == 2:
            if scores is None:
                raise ValueError('archive_seed: score_mode "table" needs scores')
            with self._ctx():
                if isinstance(scores, torch.Tensor):
                    if scores.dtype != torch.float32:
                        raise TypeError("archive_seed: scores must be a float32 tensor, not %s" % scores.dtype)
                    sc = scores.to(self.device).contiguous().view(-1)
                else:
                    sc = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32).ravel()).to(self.device)
            if len(off) and sc.numel() < int(off[-1]):
                raise ValueError("archive_seed: scores holds %d values, offsets[-1] is %d" % (sc.numel(), int(off[-1])))
        cn = None
        with self._ctx():
            if counts:
                cn = torch.zeros((len(lv), 4), dtype=torch.int32, device=self.device)
            ptr = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
            dev = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
            nat.check(self.h, self.lib.npp_archive_seed(self.h, ptr(inp) if len(inp) else None, ptr(off), ptr(lv), len(lv), mode, dev(sc),
                                                        dev(cn)))
        return cn

    def archive_select(self, mask=None):
        """For every env (mask: u8 / bool [n], None = all) draw a slot among the occupied cells of the env's level, weighted by
        1 / sqrt(visits + chosen + 1); returns the int32 CUDA tensor [n] (-1: masked out, or the level holds no cell) -- the
        `slots` argument of archive_restore."""
        m = self._cell_arg(mask, torch.uint8, "archive_select: mask")
        with self._ctx():
            slots = torch.empty(self.n, dtype=torch.int32, device=self.device)
        nat.check(self.h, self.lib.npp_archive_select(self.h, C.c_void_p(m.data_ptr()) if m is not None else None,
                                                      C.c_void_p(slots.data_ptr())))
        self._keep_archive = (m,)
        return slots

    def archive_cells(self):
        """{"cell_slot" i32 (-1 = none), "cell_score" f32, "visits", "chosen": [n_levels, 2, 25, 44] indexed (level,
        switch_activated, cell_y, cell_x); "slot_key" i32 [n_slots] (-1 = unused); "n_used" i32 [1]}: CUDA views (no copy) of the
        index's tables, valid while it lives.  visits / chosen are the u32 counters seen through int32."""
        if getattr(self, "_archive_cells", None) is None:
            p = [C.c_void_p() for _ in range(6)]
            nat.check(self.h, self.lib.npp_archive_cells_view(self.h, *[C.byref(x) for x in p]))
            K, shape = self.n_levels * CELLS_PER_LEVEL, (self.n_levels, 2, 25, 44)
            dt = (torch.int32, torch.float32, torch.int32, torch.int32)
            cells = {k: _device_tensor(p[c].value, K, dt[c], self.device).view(shape)
                     for c, k in enumerate(("cell_slot", "cell_score", "visits", "chosen"))}
            cells["slot_key"] = _device_tensor(p[4].value, self.archive_num_slots(), torch.int32, self.device)
            cells["n_used"] = _device_tensor(p[5].value, 1, torch.int32, self.device)
            self._archive_cells = cells
        return self._archive_cells

    # ---- frame stacking (include/npp_amd.h npp_set_frame_stack; the reference's FrameStackWrapper) ----------------
    def set_frame_stack(self, visual_k=0, state_k=0, padding="zero"):
        """Stack the last visual_k player_frames / state_k game_states of every env in rings of the handle (0 = off, else
        1..12; padding "zero" or "repeat").  The rings start zeroed; frame_stack_push(reset_all=True) pads them properly."""
        if padding not in ("zero", "repeat"):
            raise ValueError("padding_type must be 'zero' or 'repeat'")
        nat.check(self.h, self.lib.npp_set_frame_stack(self.h, int(visual_k), int(state_k), 1 if padding == "repeat" else 0))
        self.stack_k = (int(visual_k), int(state_k))
        self._stack_ring = [None, None]
        if getattr(self, "_aug", None) is not None:   # the augmented player_frame buffer is sized by visual_k: allocated again
            self._aug[3] = False
            self._aug_views = None

    def render_player_frame_stacked(self):
        """player_frame of every env into the frame ring (the entry the next frame_stack_push completes)."""
        nat.check(self.h, self.lib.npp_frame_stack_render(self.h))

    def frame_stack_push(self, reset_bits=0, reset_all=False, terminal_stack=None):
        """Append this step's entry (game_state from the block, the frame rendered before) to the rings and re-pad every env
        that was reset: all of them (reset_all), or those whose flags & reset_bits is set.  terminal_stack: optional f32
        CUDA tensor [N, state_k, 41] that receives each env's stack as of its terminal step (= the live stack if it was not
        reset).  Call after join() (observation overlap)."""
        t = self.out.t
        if terminal_stack is not None:
            assert terminal_stack.dtype == torch.float32 and terminal_stack.is_cuda and terminal_stack.is_contiguous()
            assert terminal_stack.shape == (self.n, self.stack_k[1], 41)
        nat.check(self.h, self.lib.npp_frame_stack_push(
            self.h, C.c_void_p(t["game_state"].data_ptr()), C.c_void_p(t["terminal_state"].data_ptr()),
            C.c_void_p(t["flags"].data_ptr()), int(reset_bits), 1 if reset_all else 0,
            C.c_void_p(terminal_stack.data_ptr()) if terminal_stack is not None else None))

    def frame_stack_views(self):
        """(player_frame [N, visual_k, 84, 84, 1] u8, game_state [N, state_k, 41] f32) CUDA views of the current windows
        (None where that key is not stacked): no copy; each env's K entries are contiguous, oldest first, envs are
        2 K entries apart.  The rings are rewritten in place, so a view shows the window of the latest push."""
        out = []
        for which, (shape, dt, esz) in enumerate((((84, 84, 1), torch.uint8, 1), ((41,), torch.float32, 4))):
            k = self.stack_k[which]
            if not k:
                out.append(None)
                continue
            base, off, stride = C.c_void_p(), C.c_int64(), C.c_int64()
            nat.check(self.h, self.lib.npp_frame_stack_view(self.h, which, C.byref(base), C.byref(off), C.byref(stride)))
            ring = self._stack_ring[which]
            if ring is None or ring[0] != base.value:   # a torch tensor over the ring memory (owned by the handle)
                ring = (base.value, _device_tensor(base.value, self.n * stride.value, dt, self.device))
                self._stack_ring[which] = ring
            e = int(np.prod(shape))
            out.append(torch.as_strided(ring[1], (self.n, k) + shape, (stride.value, e) + tuple(
                int(np.prod(shape[i + 1:])) for i in range(len(shape))), off.value))
        return tuple(out)

    # ---- frame augmentation (include/npp_amd.h npp_set_frame_augmentation; the reference's apply_augmentation) ------
    def set_frame_augmentation(self, enable=True, p=0.5, intensity="medium", seed=0):
        """Augment player_frame and global_view on the device (translate, flip, coarse dropout, brightness / contrast with the
        reference's gates; the project's own integer definition, DESIGN.md 15 -- parity with albumentations' pixels is unpinned).
        p and intensity are checked here with the reference's messages; the native switch is thrown by the next
        frame_augment(), after the frames it reads have been rendered (and after set_frame_stack), and restarts the call count
        at 0.  enable=False frees the buffers at once."""
        if not enable:
            self._aug = None
            nat.check(self.h, self.lib.npp_set_frame_augmentation(self.h, 0, 0.0, 1.0, 0))
            return
        check_frame_augmentation(p, intensity)
        self._aug = [float(p), AUG_SCALES[intensity], int(seed) & (2**64 - 1), False]   # last: the native switch was thrown
        self._aug_views = None

    def frame_augment(self, params=None):
        """One augmentation call: every env draws its parameters (params=None), or takes them from params, int32
        [N, 2, 14] (AugParams per env for player_frame and global_view; how tests reach corner parameters).  Call after join()
        and frame_stack_push().  The results are frame_augment_views()."""
        cfg = getattr(self, "_aug", None)
        if cfg is None:
            raise RuntimeError("set_frame_augmentation() first")
        if not cfg[3]:
            nat.check(self.h, self.lib.npp_set_frame_augmentation(self.h, 1, cfg[0], cfg[1], cfg[2]))
            cfg[3] = True
        ptr = None
        if params is not None:
            params = np.ascontiguousarray(params, dtype=np.int32)
            assert params.shape == (self.n, 2, AUG_WORDS)
            ptr = params.ctypes.data_as(C.c_void_p)
        code = self.lib.npp_frame_augment(self.h, ptr)
        if code == nat.NPP_ERR_INVALID:
            raise ValueError(self.lib.npp_last_error(self.h).decode())
        nat.check(self.h, code)

    def frame_augment_views(self):
        """(player_frame [N, max(K, 1), 84, 84, 1] u8, global_view [N, 176, 100, 1] u8): CUDA tensors over the handle's
        augmented buffers (no copy), rewritten by the next frame_augment()."""
        if getattr(self, "_aug_views", None) is None:
            out = []
            for which, shape in enumerate(((84, 84, 1), (176, 100, 1))):
                base, nbytes = C.c_void_p(), C.c_int64()
                nat.check(self.h, self.lib.npp_frame_augment_view(self.h, which, C.byref(base), C.byref(nbytes)))
                t = _device_tensor(base.value, nbytes.value, torch.uint8, self.device)
                out.append(t.view((self.n, -1) + shape) if which == 0 else t.view((self.n,) + shape))
            self._aug_views = tuple(out)
        return self._aug_views

    def to_host(self, names=None):
        """{name: numpy array} of the enabled outputs through ONE async device-to-host copy of the output block into pinned
        memory on the handle's stream + one synchronisation.  The arrays are views of a pinned staging block; two blocks
        alternate, so they stay valid until the to_host() call after the next one."""
        self.join()
        return self.out.to_host(self.stream, names)

    def sync(self):
        nat.check(self.h, self.lib.npp_sync(self.h))

    # ---- parity hooks -----------------------------------------------------------------------------------------
    def dump_state(self, env0=0, count=None):
        count = self.n - env0 if count is None else count
        f = np.zeros((count, nat.DUMP_F64), dtype=np.float64)
        i = np.zeros((count, nat.DUMP_I32), dtype=np.int32)
        nat.check(self.h, self.lib.npp_dump_state(
            self.h, env0, count, f.ctypes.data_as(C.POINTER(C.c_double)), i.ctypes.data_as(C.POINTER(C.c_int32))))
        return f, i

    def set_ninja_state(self, xyv, env0=0):
        """Test aid: overwrite xpos, ypos, xspeed, yspeed of envs [env0, env0 + len(xyv)) with the rows of xyv (f64 [count, 4])
        and nothing else; synchronises like dump_state().  Non-finite values raise ValueError and leave every env untouched.
        Afterwards an env's action route and archive meta rows no longer describe its state."""
        a = np.ascontiguousarray(xyv, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != 4:
            raise ValueError("set_ninja_state: xyv must be [count, 4] (x, y, vx, vy)")
        code = self.lib.npp_set_ninja_state(self.h, int(env0), len(a), a.ctypes.data_as(C.POINTER(C.c_double)))
        if code == nat.NPP_ERR_INVALID:
            raise ValueError(self.lib.npp_last_error(self.h).decode())
        nat.check(self.h, code)

    def set_mover_state(self, slot, xyab, field=None, env0=0):
        """Test aid: overwrite x, y, a, b of mover `slot` (entity_dic order) in envs [env0, env0 + len(xyab)) with the rows of xyab
        (f64 [count, 4]; a, b: speed of a bounce block / death ball, target of a drone, 0 for the thwumps) and, when `field` (int
        [count]) is given, its state (thwump -1 / 0 / 1) or dir (drone 0..3).  Cell and list-order number stay, as Entity.cell does
        after an attribute assignment in the reference.  Synchronises.  A refusal raises ValueError and writes nothing."""
        a = np.ascontiguousarray(xyab, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != 4:
            raise ValueError("set_mover_state: xyab must be [count, 4] (x, y, a, b)")
        fp = None
        if field is not None:
            f = np.ascontiguousarray(field, dtype=np.int32).ravel()
            if len(f) != len(a):
                raise ValueError("set_mover_state: one field value per row")
            fp = f.ctypes.data_as(C.POINTER(C.c_int32))
        code = self.lib.npp_set_mover_state(self.h, int(env0), len(a), int(slot), a.ctypes.data_as(C.POINTER(C.c_double)), fp)
        if code == nat.NPP_ERR_INVALID:
            raise ValueError(self.lib.npp_last_error(self.h).decode())
        nat.check(self.h, code)

    def dump_movers(self, env):
        """[n, 5] f64 rows x, y, a, b, state / dir of one env's movers in entity_dic order (see npp_dump_movers)."""
        buf = np.zeros((1024, 5), dtype=np.float64)
        n = C.c_int(0)
        nat.check(self.h, self.lib.npp_dump_movers(self.h, int(env), buf.ctypes.data_as(C.POINTER(C.c_double)), len(buf), C.byref(n)))
        return buf[: n.value].copy()

    def dump_entities(self, env):
        buf = np.zeros(4096, dtype=np.int32)
        n = C.c_int(0)
        nat.check(self.h, self.lib.npp_dump_entities(self.h, env, buf.ctypes.data_as(C.POINTER(C.c_int32)), len(buf), C.byref(n)))
        return buf[: n.value].copy()

    def dump_level_segments(self, level):
        buf = np.zeros((16384, 8), dtype=np.int16)
        n = C.c_int(0)
        nat.check(self.h, self.lib.npp_dump_level_segments(self.h, level, buf.ctypes.data_as(C.POINTER(C.c_int16)), len(buf), C.byref(n)))
        return buf[: n.value].copy()


def compile_level_segments(map_data):
    """Host-only: run the native level compiler, return (rows int16 [n,8], unsupported_mask)."""
    L = nat.lib()
    m = np.ascontiguousarray(np.asarray(map_data, dtype=np.float64))
    buf = np.zeros((16384, 8), dtype=np.int16)
    n = C.c_int(0)
    uns = C.c_uint32(0)
    nat.check(None, L.npp_compile_level_segments(
        m.ctypes.data_as(C.POINTER(C.c_double)), len(m), buf.ctypes.data_as(C.POINTER(C.c_int16)), len(buf), C.byref(n), C.byref(uns)))
    return buf[: n.value].copy(), uns.value


def compile_level_entities(map_data):
    """Host-only: rows of (kind, x, y, cell x, cell y, init) in map order."""
    L = nat.lib()
    m = np.ascontiguousarray(np.asarray(map_data, dtype=np.float64))
    buf = np.zeros((4096, 6), dtype=np.float64)
    n = C.c_int(0)
    nat.check(None, L.npp_compile_level_entities(
        m.ctypes.data_as(C.POINTER(C.c_double)), len(m), buf.ctypes.data_as(C.POINTER(C.c_double)), len(buf), C.byref(n)))
    return buf[: n.value].copy()


def reach_level_info(map_data):
    """Host-only: what the reachability table builder makes of one level: {"supported": the level is inside the restated part
    of the reference's reachability code, "nodes": len(adjacency), "mines": toggle mines, "surface_area": nodes reachable
    from the spawn (feature scale)}."""
    L = nat.lib()
    m = np.ascontiguousarray(np.asarray(map_data, dtype=np.float64))
    info = np.zeros(16, dtype=np.int32)
    nat.check(None, L.npp_reach_compile(m.ctypes.data_as(C.POINTER(C.c_double)), len(m), info.ctypes.data_as(C.c_void_p),
                                        *([None] * 11)))
    return {"supported": bool(info[0]), "nodes": int(info[1]), "mines": int(info[11]), "surface_area": int(info[13])}


def graph_tables(map_data):
    """Host-only: one level's graph observation rows (npp_graph_compile): (node_feats f32 [2500, 6], edge_index u16 [2, 20000],
    num_nodes, num_edges); the masks are 1 on the first num_nodes / num_edges entries."""
    L = nat.lib()
    m = np.ascontiguousarray(np.asarray(map_data, dtype=np.float64))
    feats = np.zeros(GRAPH_KEYS["graph_node_feats"][0], dtype=np.float32)
    edges = np.zeros(GRAPH_KEYS["graph_edge_index"][0], dtype=np.uint16)
    counts = np.zeros(2, dtype=np.int32)
    nat.check(None, L.npp_graph_compile(m.ctypes.data_as(C.POINTER(C.c_double)), len(m), feats.ctypes.data_as(C.c_void_p),
                                        edges.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p)))
    return feats, edges, int(counts[0]), int(counts[1])


def level_truncation_limit(map_data):
    """Host-only: (dynamic truncation limit in frames, reachable surface area in graph nodes) of one level."""
    L = nat.lib()
    m = np.ascontiguousarray(np.asarray(map_data, dtype=np.float64))
    lim, area = C.c_int32(0), C.c_int32(0)
    nat.check(None, L.npp_level_truncation_limit(m.ctypes.data_as(C.POINTER(C.c_double)), len(m), C.byref(lim), C.byref(area)))
    return lim.value, area.value


def level_pool_draw(weights, seed, envs, counts):
    """Host-only: the levels the pool draws for envs[i] at draw count counts[i] (include/npp_amd.h npp_set_level_pool has the
    formula).  Bad weights raise ValueError with the native message."""
    L = nat.lib()
    w = np.ascontiguousarray(weights, dtype=np.float64).ravel()
    e = np.ascontiguousarray(envs, dtype=np.int32).ravel()
    c = np.ascontiguousarray(counts, dtype=np.uint32).ravel()
    assert len(e) == len(c)
    out = np.zeros(len(e), dtype=np.int32)
    code = L.npp_level_pool_draw_host(w.ctypes.data_as(C.POINTER(C.c_double)), len(w), int(seed) & (2**64 - 1),
                                      e.ctypes.data_as(C.POINTER(C.c_int32)), c.ctypes.data_as(C.POINTER(C.c_uint32)), len(e),
                                      out.ctypes.data_as(C.POINTER(C.c_int32)))
    if code == nat.NPP_ERR_INVALID:
        raise ValueError(L.npp_last_error(None).decode())
    nat.check(None, code)
    return out


def frame_augment_params(seed, envs, counts, targets, p=0.5, intensity="medium"):
    """Host-only: the AugParams, int32 [len(envs), 14], env envs[i] draws at augmentation call counts[i] for target targets[i]
    (0 player_frame, 1 global_view): the draw the device kernel compiles (npp_augment.hpp)."""
    L = nat.lib()
    check_frame_augmentation(p, intensity)
    e = np.ascontiguousarray(envs, dtype=np.int32).ravel()
    c = np.ascontiguousarray(counts, dtype=np.uint32).ravel()
    t = np.ascontiguousarray(targets, dtype=np.int32).ravel()
    assert len(e) == len(c) == len(t)
    out = np.zeros((len(e), AUG_WORDS), dtype=np.int32)
    nat.check(None, L.npp_frame_augment_params_host(int(seed) & (2**64 - 1), float(p), AUG_SCALES[intensity], e.ctypes.data_as(C.c_void_p),
                                                    c.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), len(e),
                                                    out.ctypes.data_as(C.c_void_p)))
    return out


def frame_augment_apply(frames, params):
    """Host-only: the per-pixel function the device kernel compiles, on frames u8 [n, H, W] with params int32 [n, 14]."""
    L = nat.lib()
    f = np.ascontiguousarray(frames, dtype=np.uint8)
    q = np.ascontiguousarray(params, dtype=np.int32)
    assert f.ndim == 3 and q.shape == (f.shape[0], AUG_WORDS)
    out = np.zeros_like(f)
    code = L.npp_frame_augment_apply_host(f.ctypes.data_as(C.c_void_p), f.shape[0], f.shape[1], f.shape[2], q.ctypes.data_as(C.c_void_p),
                                          out.ctypes.data_as(C.c_void_p))
    if code == nat.NPP_ERR_INVALID:
        raise ValueError(L.npp_last_error(None).decode())
    nat.check(None, code)
    return out


def compile_level_zoo(map_data):
    """Host-only: (hor [89, 51], ver [89, 51] grid-edge counters at load, movers [n, 4] = type, x, y, creation order)."""
    lib = nat.lib()
    m = np.ascontiguousarray(np.asarray(map_data, dtype=np.float64))
    edges = np.zeros(2 * 89 * 51, dtype=np.int32)
    mov = np.zeros((1024, 4), dtype=np.float64)
    n = C.c_int(0)
    nat.check(None, lib.npp_compile_level_zoo(m.ctypes.data_as(C.POINTER(C.c_double)), len(m), edges.ctypes.data_as(C.POINTER(C.c_int32)),
                                              mov.ctypes.data_as(C.POINTER(C.c_double)), len(mov), C.byref(n)))
    return edges[: 89 * 51].reshape(89, 51), edges[89 * 51 :].reshape(89, 51), mov[: n.value].copy()
