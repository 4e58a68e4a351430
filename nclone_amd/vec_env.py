"""Gymnasium-shaped host classes over the native stepper.

  NppVecEnvironment  N environments per object; the same observation keys as the reference's NppEnvironment with a
                     leading batch dimension (nclone/gym_environment/npp_environment.py:504 reset,
                     base_environment.py:483 step).
  NppEnvironment     one environment, literal drop-in signatures: reset() -> (obs, info),
                     step(int) -> (obs, float, bool, bool, dict).
  NPlayHeadless      the facade the reference's tools drive (nclone/nplay_headless.py:28): load_map_from_map_data,
                     reset, tick(h, j), ninja_has_won/died, ninja_position, get_ninja_state, ...

Everything executes in the HIP kernels; nothing here falls back to the CPU.
"""
import numpy as np
import torch

from . import _native as nat
from . import spaces
from .engine import GRAPH_KEYS, NppBatch, _as_f64_blob, graph_tables

ACTION_TABLE = [(0, 0), (-1, 0), (1, 0), (0, 1), (-1, 1), (1, 1)]  # base_environment.py:366-402
DEATH_CAUSES = {0: None, 1: "mine", 2: "terminal_impact", 3: None}   # 3: drone / thwump / death ball / crush: kill() without a cause
MAX_TIME_IN_FRAMES = 10000   # gym_environment/constants.py:8-10


def calculate_truncation_limit(surface_area, reachable_mine_count=0):
    """Dynamic truncation limit of the reference (gym_environment/truncation_calculator.py:19-57):
    clip((sqrt(surface_area) * 20 + mines * 75) * 25, 1200, MAX_TIME_IN_FRAMES).  `surface_area` = reachable graph nodes
    (engine.level_truncation_limit computes both for a level).  The native path applies it per level by itself:
    NppVecEnvironment(truncation_limit="dynamic"), the default, = npp_set_dynamic_truncation."""
    v = (np.sqrt(surface_area) * 20.0 + reachable_mine_count * 75.0) * 25
    return int(np.clip(v, 1200, MAX_TIME_IN_FRAMES))


def level_category(tag):
    """The category a level tag of nclone_amd.levels names: the tag without its last ":"-separated field ("maze:tiny:100001" ->
    "maze:tiny", "replay:17" -> "replay")."""
    return tag.rsplit(":", 1)[0] if ":" in tag else tag


def expand_category_weights(category_weights, level_categories):
    """Per-level pool weights from per-category ones, as the reference's map loader draws: a category with probability
    proportional to its weight (env_map_loader.py:210-234), then a level of it uniformly.  category_weights: {category: weight};
    level_categories: the category of every loaded level (e.g. [level_category(t) for t in tags]).  Categories without a weight
    get 0; a weighted category without any level raises ValueError."""
    cats = list(level_categories)
    count = {}
    for c in cats:
        count[c] = count.get(c, 0) + 1
    for c, w in category_weights.items():
        if w and c not in count:
            raise ValueError("category %r has weight %r but no loaded level" % (c, w))
    return np.array([float(category_weights.get(c, 0.0)) / count[c] for c in cats], dtype=np.float64)


def route_capacity_for(record_routes, route_capacity, frame_skip, truncation_limit):
    """The `capacity` NppVecEnvironment hands to NppBatch.set_routes (0 = routes off); needs no device.  The default is the longest
    episode the env can have: its largest truncation limit ("dynamic": MAX_TIME_IN_FRAMES) divided by frame_skip, rounded up -- 2500
    actions at 10 000 frames and frame_skip 4."""
    if not record_routes:
        if route_capacity is not None:
            raise ValueError("route_capacity without record_routes=True")
        return 0
    if route_capacity is not None:
        if int(route_capacity) != route_capacity or int(route_capacity) <= 0:
            raise ValueError("route_capacity must be a positive number of actions")
        return int(route_capacity)
    limit = MAX_TIME_IN_FRAMES if isinstance(truncation_limit, str) else int(np.max(truncation_limit))
    return max(1, -(-limit // int(frame_skip)))


def controls_to_input_byte(hor, jump):
    """(hor, jump) -> replay input byte (bit0 jump, bit1 right, bit2 left; replay/replay_executor.py:61-84)."""
    return (1 if jump else 0) | (2 if hor > 0 else 0) | (4 if hor < 0 else 0)


def reduce_evaluation(levels, episodes_per_level, done, is_success, returns, frames):
    """The per-level table of an evaluation: the [J] per-job arrays (job j = episode j // L of levels[j % L]) reshaped to [K, L] and
    summed along axis 0 in float64, episode 0 first, over the jobs that are done: {"level" [L], "episodes" int64 [L], "success_rate",
    "mean_return", "mean_frames" float64 [L]; 0 where a level has no finished episode}."""
    lv = np.asarray(levels, dtype=np.int32).ravel()
    K, L = int(episodes_per_level), len(lv)
    done = np.asarray(done, dtype=bool).reshape(K, L)
    n = done.sum(axis=0, dtype=np.int64)

    def total(v):
        return np.where(done, np.asarray(v, dtype=np.float64).reshape(K, L), 0.0).sum(axis=0, dtype=np.float64)

    div = np.where(n > 0, n, 1).astype(np.float64)
    return {"level": lv.copy(), "episodes": n,
            "success_rate": np.where(n > 0, total(np.asarray(is_success, dtype=bool)) / div, 0.0),
            "mean_return": np.where(n > 0, total(returns) / div, 0.0),
            "mean_frames": np.where(n > 0, total(frames) / div, 0.0)}


class NppVecEnvironment:
    """N N++ environments stepped in lock-step on one MI355X.

    levels      sequence of raw map_data arrays (ints/floats/bytes)
    level_ids   which level each env plays (default: env i plays level (i // 64) % n_levels, so every 64-env block
                shares a level and the kernel stages it in LDS)
    output      "torch" (CUDA tensors, zero copies) or "numpy" (host copies; drop-in for numpy training loops)
    truncation_limit  "dynamic" (default; the reference env's per-level limit from the reachable surface area,
                npp_environment.py:1238-1256) or a number of frames for every env (10000 = the reference's fallback)
    The step's `reward` carries only the sparse terminal constants by default -- reward parity, sparse mode: none; pbrs mode:
    section 20 of DESIGN.md (reward_mode="pbrs" below returns the reference's PBRS reward from a device kernel).

    Frame stacking (the reference's EnvironmentConfig.frame_stack + FrameStackWrapper, frame_stack_wrapper.py):
    enable_visual_frame_stacking / visual_stack_size, enable_state_stacking / state_stack_size, frame_stack_padding_type
    ("zero" or "repeat") -- the reference config's names (config.py:22-60).  With it, obs["player_frame"] is [N, K, 84, 84, 1]
    and obs["game_state"] [N, K, 41], oldest first; every other key is unchanged.  The stack of an env is re-padded (K - 1
    padding entries, then the new observation) at reset(), at reset(options={"checkpoint": ...}) from the restored / replayed
    observation, and when the kernel auto-resets it.  Visual stacking needs enable_visual_observations (otherwise it is
    ignored, as in the reference).  The flags are taken as given, as create_evaluation_env passes them: the reference's
    create_training_env omits enable_visual_stacking, so the wrapper's default (on) applies there -- pass it explicitly.
    Sizes outside 1..12 and other paddings raise ValueError with the reference's messages.
    With state stacking, info["terminal_game_state_stack"] [N, K, 41] is, for every env reset in this step, the stack it
    would have shown at its terminal step (the previous window's last K - 1 entries, then terminal_state), else the live stack.
    output="torch": the stacked tensors are views of device rings (no copy): each env's K entries are contiguous, but envs are
    2 K entries apart, and the rings are rewritten by the next step.  output="numpy": contiguous host arrays.

    Frame augmentation (the reference's AugmentationConfig, config.py:64-87, applied by FrameStackWrapper.observation to
    player_frame and global_view at every observation, frame_stack_wrapper.py:343-377, 402-462):
    enable_augmentation=True returns both keys augmented on the device -- translate, horizontal flip, coarse dropout and
    brightness / contrast, in the reference's order and with its gates 0.8 p, 0.4 p, 0.5 p, 0.4 p (augmentation_p, default 0.5)
    and its three intensities (augmentation_intensity "light", "medium", "strong").  The pixels follow the project's own integer
    definition: PARITY WITH ALBUMENTATIONS' PIXELS IS UNPINNED (albumentations' output is not reproduced bit for bit), and the
    draws are a counter-based hash of (augmentation_seed, env index, observation count, key), not numpy's global stream;
    augmentation_seed=None takes fresh entropy, reset(seed=s) restarts the stream from s.  Every observation draws anew, reset
    observations included; all K frames of a stacked player_frame share one draw, global_view draws on its own.  Shapes and
    spaces are unchanged; the frame rings keep clean frames.  output="torch": persistent device tensors, rewritten by the next
    step.  Ignored without enable_visual_observations (nothing to act on, as in the reference); a bad intensity or p raises
    ValueError with the reference's messages.  Off by default (the reference's default is on): nothing is allocated or launched.

    Level pool (the reference's per-episode map draw, env_map_loader.py:111-208): level_weights, one non-negative
    weight per level, makes every env draw its next level -- level l with probability w[l] / sum(w) -- whenever its episode ends in
    step() (with autoreset) and in reset() (not in the checkpoint resets, which keep the level they restore).  An env that draws
    another level returns that level's spawn observation; one that draws its own level resets as without the pool.  The draws are a
    counter-based hash of (level_seed, env index, draw count), so a run is reproducible from level_seed; they do not reproduce the
    reference's Python `random` stream.  reset(seed=s) reseeds the pool with s.  set_level_weights() changes the weights between
    steps (curriculum); expand_category_weights() turns per-category weights into per-level ones.  level_weights=None (default):
    every env keeps the level level_ids gives it, as before.  info["level_id"] (both modes): the level each env plays after the step.

    Graph observations (the reference's EnvironmentConfig.enable_graph_observations): enable_graph_observations=True
    adds graph_node_feats [N, 2500, 6] f32, graph_edge_index [N, 2, 20000] u16, graph_node_mask [N, 2500] u8 and graph_edge_mask
    [N, 20000] u8, and their Boxes to observation_space.  The reference builds the graph at every reset from the loaded level and
    keeps it for the episode, so the rows are a constant of each env's level: they are rewritten only for envs whose level changed.
    output="torch": persistent device tensors updated in place (the same lifetime as the other keys).  output="numpy": two host
    buffer sets alternate, filled from host copies of the per-level tables (no per-step device-to-host copy of these 162.5 KB per
    env), so the previous step's arrays stay valid.  Not part of the terminal info.  Off by default.

    Checkpoint archive (the reference's Go-Explore checkpoints, state_checkpoint.py / base_environment.py:1769-1789):
    checkpoint_slots=S > 0 keeps S single-env states on the device.  archive_store(slot_ids) saves env e in slot slot_ids[e];
    reset(options={"checkpoint": {"slots": slot_ids}}) and restart(slot_ids) put a slot into ANY env that plays the slot's level --
    one copy instead of replaying the action sequence; archive_meta() shows each slot's position, 24 px cell, frame, level and
    switch state to a selection rule in torch.  A restored env keeps the slot's frame count (its truncation budget continues from
    the checkpoint).  Not together with level_weights (ValueError).
    checkpoint_cells=True (needs checkpoint_slots) puts Go-Explore's cell index over the archive: archive_explore(score)
    keeps the best state per (level, switch_activated, 24 px cell) in slots the index allocates itself, and
    restart_from_archive(done_mask) restarts the masked envs from slots drawn by visit count among the cells of their own level
    (checkpoint_seed seeds the draws); archive_store is refused while the index owns the slots.
    seed_archive_from_replays(replays) fills the index from recorded demonstrations before training starts, as the reference's
    DemoCheckpointSeeder does, without counting visits.

    Action routes (the reference's `_action_sequence`, base_environment.py:186 / :517 / :1677 / :2114, and what a StateCheckpoint
    is made of, state_checkpoint.py): record_routes=True keeps, on the device, the actions that led every env from
    its spawn to where it is, and the route of the episode that ended last.  get_action_sequence_length() / get_current_action_sequence(env)
    are the reference's two accessors (:2332-2349); finished_routes(mask) returns the last finished episodes (a won episode's
    solution outlives the auto-reset); with checkpoint_slots, every slot carries the route of its state: archive_routes(slot_ids)
    exports them with the StateCheckpoint fields the device knows, and restart() / reset(options={"checkpoint": {"slots": ...}})
    leave the slot's route as the env's own, as reset(options={"checkpoint": seq}) leaves seq.  route_capacity: actions per route
    (default: the longest episode the env can have, route_capacity_for; about 5 KB per env at 10 000 frames and frame_skip 4);
    longer episodes set bit 1 of the route's "bits" and drop the actions past the capacity.  replay.route_to_replay() writes a
    route as a replay file.  Off by default: nothing is allocated or launched.

    Minimal observation mode (the reference's EnvironmentConfig.observation_mode = MINIMAL, config.py:17-20):
    observation_mode="minimal" makes `obs` the reference's small observation (npp_environment.py:2232-2270): minimal_observation
    [N, 40] f32 (compute_minimal_observation, observation_processor.py:505-567: 12 physics, 8 path guidance, 4 mines x 4, 4
    buffers), action_mask [N, 6] i8 and the pass-through scalars player_x / player_y, player_won, player_dead, death_cause (the
    code of info["death_cause_code"]), switch_activated, switch_x / switch_y, exit_door_x / exit_door_y -- of the state the
    observation shows, so an env that was auto-reset reports its spawn state (not won, not dead); the reward subsystem's
    `_cached_*_distance` keys are left out.  game_state, entity_positions and the 112 / 38 / 3 / 25-float keys are not in `obs`
    and (output="numpy") not copied to the host; the 38 / 3 / 25-float outputs are not allocated.  observation_space is the
    reference's two-key Dict.  reward, terminated, truncated and info keep their meaning (info["terminal_observation"] stays the
    terminal game_state: there is NO terminal minimal observation, the reference defines none).  Options with nothing to act on
    in this mode (visual observations, either frame stacking, graph observations, enable_spatial_context / enable_reachability /
    enable_switch_states) raise ValueError, as does any other mode string; levels npp_reachability refuses (several exit switches)
    are refused at the first reset().  "full" (default): everything above, unchanged.

    Path-direction action masking (the reference env's _get_action_mask_with_path_update, base_environment.py:3075-3107, and the last
    stage of Ninja.get_valid_action_mask, ninja.py:743-800): action_masking_mode="hard" returns the action_mask the
    reference ENV returns in its default masking mode -- where the level cache's multi-hop direction from the ninja's graph node
    to the current goal is a straight path, "left" keeps NOOP and LEFT, "right" keeps NOOP and RIGHT, "down" removes the three jump
    actions -- in every observation path (reset, step, minimal mode, restart / restart_from_archive, the checkpoint options of
    reset; with frame stacking the mask is not stacked).  "soft" returns the unfiltered mask.  Both add info["path_direction"] (i8
    [N]: 0 none, 1 left, 2 right, 3 down; what a trainer's logit bias needs; not an observation key, the reference's space has
    none) to reset() and step(), and at episode end info["deterministic_mask_applied_count"] / info["deterministic_mask_rate"]
    (base_environment.py:1280-1290; [N], 0 for envs whose episode goes on): detector calls of the episode that classified from the
    graph, and their share of the episode's observations -- the project's own count, which leaves out the terminal observation an
    auto-resetting env never shows (parity of the two numbers is unpinned).  None / "none" (default): today's mask, nothing is
    launched.  set_action_masking_mode(mode) changes it between steps (the reference's annealing schedule hard -> soft -> none).
    Levels npp_reachability refuses (several exit switches) raise at the first observation with the mode on.

    Reward.  reward_mode="sparse" (default): the step kernel's three constants, reward parity with the
    reference: none.  reward_mode="pbrs": `reward` is the reference's RewardCalculator.calculate_reward (main_reward_calculator.py:
    225-904 with RewardConfig(enable_path_waypoints=False), no goal curriculum): potential-based shaping on path distance with the
    reference's position cache, distance and switch milestones, time penalty, completion-approach bonus, terminal rewards, times
    0.1 -- from a device kernel behind the step, in both output modes and without auto-reset too; parity: section 20.
    info["pbrs_components"] ([N, 6] f32, unscaled: pbrs, distance milestone, switch milestone, approach bonus, terminal, potential)
    goes with it.  reward_params: a dict with some of death_penalty, level_completion_reward, switch_activation_reward,
    time_penalty_per_step, pbrs_objective_weight, pbrs_gamma (defaults: a fresh RewardConfig()); set_reward_params(**kw) changes
    them between steps (the reference's schedules are the caller's business).  Every episode start -- auto-reset, reset(),
    restart() / restart_from_archive(), the checkpoint options of reset (a sequence replay runs with the mode off and restarts the
    reward state on the state it ends in) -- restarts the env's reward state.  One deviation: the last step of an episode that ends by
    TRUNCATION under auto-reset carries time penalty + switch milestone only (the reference evaluates the final position, which the
    in-kernel reset has overwritten).  The reward launch follows the observation kernels, so obs_overlap keeps its effect.  Levels the mode refuses (those npp_reachability
    refuses, and those on which the reference itself raises "Combined geometric path distance is infinite") raise NppError in
    the constructor.
    reward_waypoints=True (needs reward_mode="pbrs"): the sequential path waypoints of a fresh RewardConfig()
    (enable_path_waypoints=True, the reference's default) -- waypoints every 12 px along the two optimal paths, a bonus for
    collecting the next one, less out of sequence -- added to `reward` where the reference adds it.  info["waypoints"] holds the
    step's unscaled bonus, the collected sequence index (-1: none), the next expected index and the collected count.
    waypoint_params: a dict with some of collection_radius (at most 24), out_of_order_scale, progress_scale, progress_spacing
    (defaults: 18, 0.3, 2.0, 12); set_waypoint_params(**kw) changes the first three between steps; level_waypoints(level) returns a
    level's table.  Levels whose paths carry more than 512 waypoints raise NppError in the constructor.
    episode_stats=True: per-env episode records and a per-level outcome table, kept by a device kernel behind every
    step.  info["_episode"] is a bool [N], true where an episode ended in this step, and info["episode"] holds, per env, the episode
    that ended last (rows outside the mask: the env's previous one; before its first: zeros, level_id -1): "r" the return (float64,
    the sum of the step rewards in step order), "l" its frames (the reference's sim.frame), "steps", "is_success",
    "switch_activated", "switch_activation_frame" (the episode's frame count after the step that activated the switch, -1 = never:
    step granularity, where the reference has the exact tick -- the one deviation), "level_id", "from_checkpoint" (begun by a
    checkpoint restore or replay), and with reward_mode="pbrs" "pbrs_total" and "terminal_reward".  output="torch": views of the
    handle's planes, rewritten by the next step.  episode_level_stats() returns the table by column with success_rate and
    mean_return per level -- a curriculum's input for set_level_weights(); reset_episode_level_stats() zeroes it.
    """

    metadata = {"render_modes": []}

    def __init__(self, levels, num_envs, level_ids=None, frame_skip=4, device=0, enable_visual_observations=False,
                 truncation_limit="dynamic", output="torch", autoreset=True, enable_spatial_context=False,
                 enable_switch_states=False, fast_reset=True, stream=None, enable_reachability=False, obs_overlap=0,
                 enable_visual_frame_stacking=False, visual_stack_size=4, enable_state_stacking=False, state_stack_size=4,
                 frame_stack_padding_type="zero", level_weights=None, level_seed=None, enable_graph_observations=False,
                 observation_mode="full", enable_augmentation=False, augmentation_p=0.5, augmentation_intensity="medium",
                 augmentation_seed=None, checkpoint_slots=0, checkpoint_cells=False, checkpoint_seed=0, record_routes=False,
                 route_capacity=None, action_masking_mode=None, reward_mode="sparse", reward_params=None, reward_waypoints=False,
                 waypoint_params=None, episode_stats=False, goal_curriculum=False, goal_curriculum_params=None):
        assert output in ("torch", "numpy")
        self._episode = bool(episode_stats)
        self._sweep = False    # an evaluation is running (start_evaluation)
        self._swept = False    # one has run: the levels moved on the device and the fixed assignment no longer describes them
        self._goal = bool(goal_curriculum)
        self._goal_params = dict(goal_curriculum_params) if goal_curriculum_params else {}
        if self._goal and reward_waypoints:
            raise ValueError("goal_curriculum with reward_waypoints=True: the waypoints towards the moved goals are not computed "
                             "(DESIGN.md 25); reward_mode=\"pbrs\" without them runs on the variant levels")
        if self._goal and enable_graph_observations:   # no fixture pins the graph rows of a variant level
            raise ValueError("goal_curriculum with enable_graph_observations: graph observations are not served on the curriculum's "
                             "variant levels (npp_graph_observation refuses them)")
        if reward_mode not in ("sparse", "pbrs"):
            raise ValueError('reward_mode must be "sparse" or "pbrs", not %r' % (reward_mode,))
        self._pbrs = reward_mode == "pbrs"
        self._reward_params = dict(reward_params) if reward_params else {}
        if reward_waypoints and not self._pbrs:
            raise ValueError('reward_waypoints=True needs reward_mode="pbrs": the waypoint bonus is a term of that reward')
        self._waypoints = bool(reward_waypoints)
        self._waypoint_params = dict(waypoint_params) if waypoint_params else {}
        if action_masking_mode not in (None, "none", "hard", "soft"):
            raise ValueError('action_masking_mode must be None, "none", "hard" or "soft", not %r' % (action_masking_mode,))
        self._mask_on = action_masking_mode in ("hard", "soft")
        if int(checkpoint_slots) < 0:
            raise ValueError("checkpoint_slots must be >= 0")
        self.route_capacity = route_capacity_for(record_routes, route_capacity, frame_skip, truncation_limit)
        if checkpoint_cells and not checkpoint_slots:
            raise ValueError("checkpoint_cells needs checkpoint_slots > 0 (the cell index allocates the archive's slots)")
        if checkpoint_slots and level_weights is not None:
            raise ValueError("checkpoint_slots with level_weights: with the level pool on, levels move on the device and a "
                             "checkpoint record's level can no longer be matched to its env (DESIGN.md 16)")
        spaces.check_frame_augmentation(augmentation_p, augmentation_intensity)
        self._minimal = spaces.check_observation_mode(
            observation_mode, enable_visual_observations=enable_visual_observations,
            enable_visual_frame_stacking=enable_visual_frame_stacking, enable_state_stacking=enable_state_stacking,
            enable_graph_observations=enable_graph_observations, enable_spatial_context=enable_spatial_context,
            enable_reachability=enable_reachability, enable_switch_states=enable_switch_states,
            enable_augmentation=enable_augmentation)
        spaces.check_frame_stack(visual_stack_size, state_stack_size, frame_stack_padding_type)
        self.num_envs = int(num_envs)
        self.frame_skip = int(frame_skip)
        self.output = output
        self.enable_visual_observations = bool(enable_visual_observations)
        # stack sizes, 0 = not stacked (visual stacking applies only when player_frame is observed, frame_stack_wrapper.py:190)
        self._vk = int(visual_stack_size) if enable_visual_frame_stacking and self.enable_visual_observations else 0
        self._sk = int(state_stack_size) if enable_state_stacking else 0
        self.single_action_space = spaces.action_space()
        self.single_observation_space = spaces.observation_space(self.enable_visual_observations,
                                                                 spatial_context=bool(enable_spatial_context),
                                                                 switch_states=bool(enable_switch_states),
                                                                 reachability=bool(enable_reachability),
                                                                 visual_stack=self._vk, state_stack=self._sk,
                                                                 graph=bool(enable_graph_observations), minimal=self._minimal)
        self.action_space = self.single_action_space
        self.observation_space = self.single_observation_space
        outputs = ["positions"]
        if self._minimal:
            outputs.append("minimal_observation")
        if enable_spatial_context:
            outputs.append("spatial_context")
        if enable_switch_states:
            outputs.append("switch_states")
        if self.enable_visual_observations:   # (a stacked player_frame lives in the handle's ring, not in the output block)
            outputs += ["global_view"] if self._vk else ["player_frame", "global_view"]
        if enable_reachability:   # reachability_features + mine_sdf_features (npp_environment.py observation keys)
            outputs += ["reachability_features", "mine_sdf_features"]
        if self._mask_on:
            outputs.append("path_direction")
        if self._pbrs:   # (the last field of the block)
            outputs.append("reward_components")
        # same-level resets are Simulator.fast_reset in the reference's env (npp_environment.py:541-557): the default here
        self._b = NppBatch(self.num_envs, device=device, autoreset=autoreset, outputs=outputs, fast_reset=fast_reset,
                           stream=stream)
        self._b.load_levels(levels)
        if self._goal:   # first: switching it on reloads the level set with one variant level per (level, stage)
            self._b.set_goal_curriculum(True, **self._goal_params)
        self._levels, self._map_ids = levels, None   # (seed_archive_from_replays matches replays to levels by map bytes)
        if level_ids is None:
            level_ids = (np.arange(self.num_envs) // 64) % len(levels)
        self._b.assign_levels(level_ids)
        if isinstance(truncation_limit, str):
            if truncation_limit != "dynamic":
                raise ValueError('truncation_limit: a number of frames or "dynamic"')
            self._b.set_dynamic_truncation(True)
        else:
            self._b.set_truncation_limit(truncation_limit)
        self._obs_overlap = bool(obs_overlap)
        if obs_overlap:   # speed knob (same bits): observation kernels of the cheap envs beside the step's expensive tail
            self._b.set_obs_overlap(int(obs_overlap))
        self._pool = level_weights is not None
        self._level_seed = None
        if self._pool:
            self._level_seed = int(level_seed) if level_seed is not None else int(np.random.SeedSequence().entropy) & (2**64 - 1)
            self._b.set_level_pool(level_weights, self._level_seed)
            self._level_ids = None
        elif self._goal:   # (levels move on the device here too)
            self._level_ids = None
        else:
            with self._b._ctx():   # the fixed assignment, for info["level_id"]
                self._level_ids_np = self._b.env_levels()
                self._level_ids = torch.from_numpy(self._level_ids_np).to(self._b.device)
        self._rng = np.random.default_rng()
        with self._b._ctx():
            self._actions = torch.zeros(self.num_envs, dtype=torch.uint8, device=self._b.device)
        self._reset_bits = 11 if autoreset else 0
        self._obs_names = ["game_state", "action_mask", "entity_pos", "positions", "flags"] + [k for k in outputs[1:] if k != "reward_components"]
        if self._minimal:   # (the packed block keeps game_state and entity_pos in front; they are neither returned nor copied)
            self._obs_names = ["action_mask", "positions", "flags", "minimal_observation"] + (["path_direction"] if self._mask_on else [])
        self._autoreset = bool(autoreset)
        if self._mask_on:
            self._b.set_action_masking(action_masking_mode)
        if self._waypoints:
            with self._b._ctx():
                self._wp_bonus = torch.zeros(self.num_envs, dtype=torch.float32, device=self._b.device)
                self._wp_info = torch.full((self.num_envs, 3), -1, dtype=torch.int32, device=self._b.device)
        self._pbrs_on()
        self._term_stack = None
        if self._vk or self._sk:
            self._b.set_frame_stack(self._vk, self._sk, frame_stack_padding_type)
            if self._sk:
                with self._b._ctx():
                    self._term_stack = torch.zeros((self.num_envs, self._sk, 41), dtype=torch.float32, device=self._b.device)
            self._host_stack = {}   # name -> [pinned buffer, pinned buffer, next]: host copies alternate like the output block's
        self._graph = None
        if enable_graph_observations:
            self._graph = _HostGraphRows(levels, self.num_envs) if output == "numpy" else {}
        # augmentation acts on the two visual keys only (without them the wrapper has nothing to act on)
        self._aug = bool(enable_augmentation) and self.enable_visual_observations
        if self._aug:
            self._aug_cfg = (float(augmentation_p), augmentation_intensity)
            seed = int(augmentation_seed) if augmentation_seed is not None else int(np.random.SeedSequence().entropy)
            self._b.set_frame_augmentation(True, *self._aug_cfg, seed=seed)
            self._obs_names = [k for k in self._obs_names if k not in ("player_frame", "global_view")]   # (numpy: the clean frames stay on the device)
            if not hasattr(self, "_host_stack"):
                self._host_stack = {}
        self.checkpoint_slots = int(checkpoint_slots)
        if self.route_capacity:   # (before the archive: its records then carry each slot's route)
            self._b.set_routes(self.route_capacity)
        if self.checkpoint_slots:
            self._b.archive_create(self.checkpoint_slots)
            with self._b._ctx():
                self._env_ids = torch.arange(self.num_envs, dtype=torch.int32, device=self._b.device)
                self._obs_flags = torch.zeros(self.num_envs, dtype=torch.uint8, device=self._b.device)
        self.checkpoint_cells = bool(checkpoint_cells)
        self.last_restart_slots = None
        if self.checkpoint_cells:
            self._b.archive_cells_create(seed=checkpoint_seed)
        if self._episode:
            self._b.set_episode_stats(True)
            with self._b._ctx():
                self._ep_ended = torch.zeros(self.num_envs, dtype=torch.uint8, device=self._b.device)

    # -- helpers ------------------------------------------------------------------------------------------------
    def _produce(self, reset_all=False):
        """Launch the secondary observation kernels (frames, switch_states) on the handle's stream, then (frame stacking)
        push this observation onto the stacks: re-padding every env when reset_all, else the envs the kernel auto-reset."""
        b = self._b
        fused = "switch_states" in b.out.t and "reachability_features" in b.out.t   # one launch writes both
        if "switch_states" in b.out.t and not fused:
            b.switch_states()
        if "player_frame" in b.out.t:
            b.render_player_frame()
            b.render_global_view()
        elif self._vk:
            b.render_player_frame_stacked()
            b.render_global_view()
        if "reachability_features" in b.out.t:
            b.reachability(with_switch_states=fused)
        if self._minimal:
            b.minimal_observation()
        b.join()   # (obs_overlap) the handle's stream waits for the kernels that went to the second stream
        if self._graph is not None and self.output == "torch":
            self._graph = b.graph_observation()
        if self._vk or self._sk:
            b.frame_stack_push(self._reset_bits, reset_all, None if reset_all else self._term_stack)
        if self._aug:   # (after the push: the padding of reset envs is in the ring)
            b.frame_augment()
        if self._mask_on:   # the detector, and in hard mode the filter on the block's action_mask, ahead of any host copy
            b.path_action_mask()

    def _stacked(self, src, with_terminal=False):
        """src with the stacked windows in place of player_frame / game_state (+ terminal_game_state_stack).  Device views for
        output="torch"; for output="numpy" the copies into pinned memory are only enqueued here -- the caller's to_host()
        synchronises the stream."""
        if not (self._vk or self._sk or self._aug):
            return src
        pf, gs = self._b.frame_stack_views() if (self._vk or self._sk) else (None, None)
        stk = {}
        if pf is not None:
            stk["player_frame"] = pf
        if gs is not None:
            stk["game_state"] = gs
            if with_terminal:
                stk["terminal_game_state_stack"] = self._term_stack
        if self._aug:   # the augmented copies take the place of both visual keys
            apf, agv = self._b.frame_augment_views()
            stk["player_frame"] = apf if self._vk else apf[:, 0]
            stk["global_view"] = agv
        if self.output == "numpy":
            with self._b._ctx():
                for k, t in stk.items():
                    slot = self._host_stack.get(k)
                    if slot is None:
                        slot = self._host_stack[k] = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for _ in range(2)] + [0]
                    host = slot[slot[2]]
                    slot[2] ^= 1
                    host.copy_(t, non_blocking=True)
                    stk[k] = host.numpy()
        out = dict(src)
        out.update(stk)
        return out

    def _obs(self, src):
        """src: {name: tensor-or-array} (device tensors, or the host views of ONE staged copy)."""
        pos = src["positions"]
        if self._minimal:   # npp_environment.py:2232-2270; scalars of the state the observation shows (spawn state after an auto-reset)
            live = (src["flags"] & self._reset_bits) == 0
            return {
                "minimal_observation": src["minimal_observation"],
                "action_mask": src["action_mask"],
                "player_x": pos[:, 0], "player_y": pos[:, 1],
                "player_won": ((src["flags"] & 1) != 0) & live, "player_dead": ((src["flags"] & 2) != 0) & live,
                "death_cause": ((src["flags"] >> 4) & 3) * live,
                "switch_activated": ((src["flags"] & 4) != 0) & live,
                "switch_x": pos[:, 2], "switch_y": pos[:, 3], "exit_door_x": pos[:, 4], "exit_door_y": pos[:, 5],
            }
        obs = {
            "game_state": src["game_state"],
            "action_mask": src["action_mask"],
            "entity_positions": src["entity_pos"],
            # pass-through scalars of the raw observation (observation_processor.py:374-399), unrounded fp64
            "player_x": pos[:, 0], "player_y": pos[:, 1], "switch_x": pos[:, 2], "switch_y": pos[:, 3],
            "exit_door_x": pos[:, 4], "exit_door_y": pos[:, 5],
            # flags describe the step that just ran; an env that was auto-reset (terminated / truncated) returns the spawn
            # observation, whose switch is not yet hit
            "switch_activated": ((src["flags"] & 4) != 0) & ((src["flags"] & self._reset_bits) == 0),
        }
        for k in ("spatial_context", "switch_states", "player_frame", "global_view", "reachability_features", "mine_sdf_features"):
            if k in src:
                obs[k] = src[k]
        return obs

    # -- Gymnasium surface ----------------------------------------------------------------------------------------
    def reset(self, seed=None, options=None):
        """Reset every env to its level's spawn state (npp_environment.py:504).  The first reset of a level assignment is
        Simulator.reset (nsim.py:62); later ones are Simulator.fast_reset (nsim.py:78) unless fast_reset=False.

        seed     seeds `action_space_sample()` (and reseeds the level pool and the frame augmentation, when on): the reference's
                 seed picks the next map (env_map_loader.py), here the levels are assigned explicitly, and the simulation itself
                 has no randomness.
        options  {"checkpoint": c} restores a Go-Explore checkpoint (base_environment.py:1769-1789, _reset_to_checkpoint):
                 c = "snapshot" puts back the state saved by `snapshot()` (a device-side copy: what the replay below would
                 reproduce, bit for bit); otherwise c (or c["action_sequence"] / c.action_sequence) is the action sequence to
                 replay from the spawn -- one sequence for every env, or an [N, K] array -- frame_skip ticks per action like
                 ActionReplayer.replay_to_checkpoint; c.source_frame_skip / c["source_frame_skip"] overrides the tick count.
                 c = {"slots": slot_ids} (checkpoint_slots > 0) restarts every env from the checkpoint archive: env e from slot
                 slot_ids[e]; with -1, or where the restore's status is not 0 (empty slot, another level, out of range), the env
                 does an ordinary spawn reset.  info = {"checkpoint_replay": False, "restored": bool [N], "restore_status": i32 [N]}.
                 Other keys of the reference (skip_map_load, new_level, map_name) concern its map loader and are ignored."""
        if self._sweep:
            raise RuntimeError("reset() in the middle of an evaluation: the sweep hands out the levels and a reset env's job would "
                               "be played twice (start_evaluation() begins a new one, stop_evaluation() ends it)")
        if seed is not None:
            self._rng = np.random.default_rng(seed)
            if self._pool:   # the pool's draws restart from the seed (off and on again: the draw counts restart at 0)
                self._level_seed = int(seed) & (2**64 - 1)
                w = self._level_weights_now
                self._b.set_level_pool(None)
                self._b.set_level_pool(w, self._level_seed)
            if self._aug:   # the augmentation stream restarts from the seed (observation count 0)
                self._b.set_frame_augmentation(True, *self._aug_cfg, seed=int(seed))
        ckpt = (options or {}).get("checkpoint")
        info = {}
        if isinstance(ckpt, dict) and "slots" in ckpt:
            self._b.reset()
            status = self._archive_restore(ckpt["slots"])
            info = {"checkpoint_replay": False, "restored": self._host(status == 0), "restore_status": self._host(status)}
        elif isinstance(ckpt, str):
            if ckpt != "snapshot":
                raise ValueError('options["checkpoint"]: "snapshot", an action sequence, or an object with .action_sequence')
            self._b.restore()
            info = {"checkpoint_replay": False, "restored_snapshot": True}
        else:
            if self._pool and ckpt is None:   # every env draws its level (the checkpoint replay keeps the one it replays on)
                self._b.draw_levels()
            self._b.reset()
            if ckpt is not None:
                seq = ckpt.get("action_sequence") if isinstance(ckpt, dict) else getattr(ckpt, "action_sequence", ckpt)
                fs = ckpt.get("source_frame_skip") if isinstance(ckpt, dict) else getattr(ckpt, "source_frame_skip", None)
                seq = np.asarray(seq if seq is not None else [], dtype=np.uint8)
                if seq.ndim == 1:
                    seq = np.broadcast_to(seq[None, :], (self.num_envs, len(seq)))
                if seq.ndim != 2 or seq.shape[0] != self.num_envs:
                    raise ValueError("checkpoint action_sequence: [K] or [num_envs, K]")
                K = int(seq.shape[1])
                if K and self._goal:
                    raise ValueError("reset(options={'checkpoint': action sequence}) with goal_curriculum: the replay is one launch of "
                                     "several steps, which the curriculum's bookkeeping refuses (DESIGN.md 25)")
                if K:
                    fs = self.frame_skip if fs is None else int(fs)
                    with self._b._ctx():
                        acts = torch.from_numpy(np.ascontiguousarray(seq.T)).to(self._b.device)
                    mode = self._b._masking   # (action masking) the replay's inner steps have no observation: the detector
                    if mode:                  # runs once, in _produce() below, on the state the replay ends in
                        self._b.set_action_masking(0)
                    if self._pbrs:            # (reward mode "pbrs") likewise: off around the replay, and switched on again on the
                        self._b.set_reward_mode("sparse")   # state the replay ends in, which restarts every env's reward state
                    try:
                        flags, _rew, frames = self._b.step_many(acts, fs)
                    finally:
                        if mode:
                            self._b.set_action_masking(mode)
                        self._pbrs_on()
                    info = {"checkpoint_replay": True, "replay_frames": frames.to(torch.int64).sum(dim=0),
                            "replay_terminated": (flags & 3).ne(0).any(dim=0)}
                    if self._episode:   # the replay's steps are not accumulated: the episode begins where it ends
                        self._b.episode_restart(None, from_restore=True)
                else:
                    info = {"checkpoint_replay": False, "replay_frames": 0}
        return self._reset_return(info)

    def _reset_return(self, info):
        """(obs, info) of the state every env is in now, every frame stack re-padded: what reset() and start_evaluation() return"""
        self._b.observe()
        self._produce(reset_all=True)
        if self.output == "torch":
            if self._mask_on:
                info["path_direction"] = self._b.out.t["path_direction"]
            return self._with_graph(self._obs(self._stacked(self._b.out.t))), info
        stk = self._stacked({})
        src = self._b.to_host(self._obs_names)
        src.update(stk)
        if self._mask_on:
            info["path_direction"] = src["path_direction"]
        return self._with_graph(self._obs(src)), info

    def _pbrs_on(self):
        """reward_mode="pbrs": the mode, and with reward_waypoints the path waypoints, switched on (again): every env's reward and
        waypoint state restarts on the state it is in"""
        if self._pbrs:
            self._b.set_reward_mode("pbrs", self._reward_params)
            if self._waypoints:
                self._b.set_reward_waypoints(True, self._waypoint_params)

    def set_waypoint_params(self, **kw):
        """reward_waypoints=True: new values for collection_radius, out_of_order_scale or progress_scale (the constructor's
        waypoint_params), from the next step on.  progress_spacing belongs to the levels' tables and cannot change here."""
        if not self._waypoints:
            raise RuntimeError("set_waypoint_params: this env was created with reward_waypoints=False")
        if "progress_spacing" in kw:
            raise ValueError("set_waypoint_params: progress_spacing is fixed when the waypoint tables are built (the constructor's waypoint_params)")
        p = dict(self._waypoint_params)
        p.update(kw)
        self._b.set_waypoint_params(p)   # (raises ValueError for an unknown name)
        self._waypoint_params = p

    def level_waypoints(self, level):
        """reward_waypoints=True: (xy f64 [count, 2] world pixels, phase u8 [count]: 0 pre-switch, 1 post-switch) of a level, in the
        order the bonus counts them."""
        if not self._waypoints:
            raise RuntimeError("level_waypoints: this env was created with reward_waypoints=False")
        return self._b.level_waypoints(level)

    def set_reward_params(self, **kw):
        """reward_mode="pbrs": new values for some of the six reward parameters (the constructor's reward_params), from the next
        step on."""
        if not self._pbrs:
            raise RuntimeError('set_reward_params: this env was created with reward_mode="sparse"')
        p = dict(self._reward_params)
        p.update(kw)
        self._b.set_reward_params(p)   # (raises ValueError for an unknown name)
        self._reward_params = p

    def set_action_masking_mode(self, mode):
        """None / "none", "hard" or "soft" (the constructor's action_masking_mode), from the next observation on.  The first
        switch to "hard" / "soft" of an env created without it re-allocates the output block: tensors returned earlier are stale."""
        if mode not in (None, "none", "hard", "soft"):
            raise ValueError('action_masking_mode must be None, "none", "hard" or "soft", not %r' % (mode,))
        on = mode in ("hard", "soft")
        if on and "path_direction" not in self._b.out.t:
            self._b.enable_outputs("path_direction")
            self._obs_names.append("path_direction")
        self._b.set_action_masking(mode)
        self._mask_on = on

    def _mask_info(self, src, done):
        """info keys of the action masking: the direction, and for envs whose episode ended the two counters' numbers."""
        numpy = self.output == "numpy"
        out = {"path_direction": src["path_direction"]}
        if numpy and not done.any():
            out["deterministic_mask_applied_count"] = np.zeros(self.num_envs, dtype=np.int64)
            out["deterministic_mask_rate"] = np.zeros(self.num_envs, dtype=np.float64)
            return out
        st = self._b.path_mask_stats()
        with self._b._ctx():
            # with auto-reset the kernel latched both at this observation; without, the episode's terminal observation is the last counted
            cnt, tot = (st["last_applied"], st["last_observed"]) if self._autoreset else (st["applied"], st["observed"])
            d = torch.as_tensor(done, device=self._b.device) if numpy else done
            cnt = torch.where(d, cnt, torch.zeros_like(cnt)).to(torch.int64)
            rate = torch.where(d, cnt.to(torch.float64) / tot.clamp(min=1).to(torch.float64), torch.zeros((), dtype=torch.float64, device=self._b.device))
            if numpy:
                cnt, rate = cnt.cpu().numpy(), rate.cpu().numpy()
        out["deterministic_mask_applied_count"], out["deterministic_mask_rate"] = cnt, rate
        return out

    @property
    def _level_weights_now(self):
        return self._b._pool_weights

    def set_level_weights(self, weights):
        """New pool weights (one per level), used from the next draw on; the draw counts and the seed are kept."""
        if not self._pool:
            raise RuntimeError("set_level_weights: this env was created without level_weights (no level pool)")
        self._b.set_level_pool(weights, self._level_seed)

    # ---- goal curriculum (the reference's set_curriculum_stage, base_environment.py:404-481) -------------
    def set_curriculum_stage(self, stage, level=None):
        """The stage of one base level (or of all): deferred to every env's next episode start, clamped to the last stage."""
        if not self._goal:
            raise RuntimeError("set_curriculum_stage: this env was created without goal_curriculum")
        self._b.goal_set_stage(stage, level)

    def goal_curriculum_state(self):
        """Per base level: stage, num_stages, window_fill, wins (int arrays [L]) and positions [L, 4], the switch x, y and door x, y of
        the level's current stage (the original ones for a level without stages).  Synchronises."""
        if not self._goal:
            raise RuntimeError("goal_curriculum_state: this env was created without goal_curriculum")
        g = self._b.goal_views()
        with self._b._ctx():
            lv = g["level_words"].cpu().numpy()
        pos = np.zeros((g["n_base"], 4))
        for l in range(g["n_base"]):
            ns, _d, orig, p = self._goal_table(l)
            pos[l] = p[lv[0, l]] if ns > 0 else orig
        return {"stage": lv[0].copy(), "num_stages": lv[2].copy(), "window_fill": lv[4].copy(), "wins": lv[6].copy(), "positions": pos}

    def _goal_table(self, level):
        if not hasattr(self, "_goal_tables"):
            self._goal_tables = {}
        if level not in self._goal_tables:
            self._goal_tables[level] = self._b.goal_stage_positions(level)
        return self._goal_tables[level]

    def _goal_rows(self):
        """per row of the level set (base levels and variants): num_stages of its base level, the positions it plays, the originals"""
        if not hasattr(self, "_goal_row_tables"):
            g = self._b.goal_views()
            nl = len(g["base_of"])
            ns, cur, orig = np.zeros(nl, dtype=np.int32), np.zeros((nl, 4)), np.zeros((nl, 4))
            for r in range(nl):
                n, _d, o, p = self._goal_table(int(g["base_of"][r]))
                ns[r], orig[r] = n, o
                cur[r] = p[g["stage_of"][r]] if g["stage_of"][r] >= 0 else o
            self._goal_row_tables = (ns, cur, orig)
        return self._goal_row_tables

    def _goal_info(self, raw_levels):
        """info["goal_curriculum"]: the fields of get_curriculum_info (intermediate_goal_manager.py:1044-1095) kept here, per env.
        One copy of the level row and of the counters to the host (synchronises, also under output="torch"), then table look-ups."""
        g = self._b.goal_views()
        with self._b._ctx():
            raw = raw_levels.cpu().numpy() if torch.is_tensor(raw_levels) else np.asarray(raw_levels)
            env = g["env_words"][:3].cpu().numpy()
        ns_row, cur_row, orig_row = self._goal_rows()
        base, stage = g["base_of"][raw], np.maximum(g["stage_of"][raw], 0)
        ns, cur, orig = ns_row[raw], cur_row[raw], orig_row[raw]
        return base.astype(np.int32), {
            "unified_stage": stage.astype(np.int32), "num_stages": ns, "stage_distance_interval": g["interval"],
            "curriculum_switch_pos": cur[:, :2], "curriculum_exit_pos": cur[:, 2:], "original_switch_pos": orig[:, :2],
            "original_exit_pos": orig[:, 2:], "episode_count": env[0], "switch_activation_count": env[1],
            "completion_count": env[2], "at_final_stage": (ns > 0) & (stage >= ns - 1)}

    def _level_id(self, numpy):
        if self._pool or self._goal or self._swept:
            if numpy:
                return self._b.env_levels()
            with self._b._ctx():
                return self._b.env_level_view().clone()
        return self._level_ids_np.copy() if numpy else self._level_ids

    def _with_graph(self, obs, levels=None):
        """obs plus the graph keys (enable_graph_observations): the device tensors (torch), or the host buffer set of this
        observation, brought up to the levels the envs play (numpy)."""
        if self._graph is None:
            return obs
        if self.output == "torch":
            obs.update(self._graph)
        else:
            obs.update(self._graph.update(self._level_id(True) if levels is None else levels))
        return obs

    def snapshot(self):
        """Save the state of every env on the device (one slot); reset(options={"checkpoint": "snapshot"}) restores it."""
        self._b.snapshot()

    # -- checkpoint archive ------------------------------------------------------------------------
    def _host(self, t):
        return t if self.output == "torch" else t.cpu().numpy()

    def _slot_list(self, slot_ids, what):
        """slot_ids [N] as the `slots` argument of the batch's archive calls (a tensor stays on the device)."""
        if not self.checkpoint_slots:
            raise RuntimeError("%s: this env was created without checkpoint_slots (no checkpoint archive)" % what)
        if isinstance(slot_ids, torch.Tensor):
            with self._b._ctx():
                slot_ids = slot_ids.to(device=self._b.device, dtype=torch.int32)
        else:
            slot_ids = np.asarray(slot_ids)
        if slot_ids.ndim != 1 or len(slot_ids) != self.num_envs:
            raise ValueError("%s: slot_ids must be [num_envs]" % what)
        return slot_ids

    def _archive_restore(self, slot_ids):
        slots = self._slot_list(slot_ids, "checkpoint restore")
        envs = self._env_ids if isinstance(slots, torch.Tensor) else np.arange(self.num_envs, dtype=np.int32)
        return self._b.archive_restore(envs, slots, status=True)

    def archive_store(self, slot_ids):
        """Store env e's state in slot slot_ids[e] of the checkpoint archive ([N]; -1 = do not store; an int32 CUDA tensor stays
        on the device, an array is checked for a slot that comes twice).  Returns the status i32 [N]: 0 stored, 1 skipped,
        4 slot out of range."""
        slots = self._slot_list(slot_ids, "archive_store")
        if self.checkpoint_cells:
            raise RuntimeError("archive_store: the cell index owns the slots (checkpoint_cells=True); archive_explore() stores")
        envs = self._env_ids if isinstance(slots, torch.Tensor) else np.arange(self.num_envs, dtype=np.int32)
        return self._host(self._b.archive_store(envs, slots, status=True))

    def archive_meta(self):
        """The archive's per-slot rows (NppBatch.archive_meta): CUDA views named by column, for a selection rule in torch."""
        return self._b.archive_meta()

    def _restart_refusal(self):
        if self._vk or self._sk or self._aug:
            raise NotImplementedError("restart() with frame stacking / frame augmentation: the frame rings and the augmentation's "
                                      "draw counters advance per observation; use reset(options={'checkpoint': {'slots': ...}})")

    def restart(self, slot_ids):
        """Between two steps: env e restarts from slot slot_ids[e] of the checkpoint archive; -1 leaves it alone.  The usual use
        follows a step whose auto-reset put the finished envs at their spawn: restart(where(done, chosen, -1)).  Returns the
        observation dict of all envs: the rows of untouched envs (and of envs whose slot was empty, of another level or out of
        range) equal what the preceding step() / reset() returned, the rows of restarted envs show the restored state; the
        step's reward, terminated, truncated and info stay as they were returned.
        Raises NotImplementedError with frame stacking or frame augmentation: the rings and the draw counters advance per
        observation, so a second observation of the untouched envs is not neutral there -- use
        reset(options={"checkpoint": {"slots": slot_ids}}), which re-pads every stack.
        With action masking on, this second observation of the step runs the detector again for every env, so the masking
        counters (info["deterministic_mask_rate"]) count the untouched envs' observation twice."""
        self._restart_refusal()
        b = self._b
        status = self._archive_restore(slot_ids)
        b.observe(flags_out=self._obs_flags)
        with b._ctx():   # the flags of restarted envs describe the restored state; the others keep the step's
            b.flags.copy_(torch.where(status == 0, self._obs_flags, b.flags))
        self._produce()
        if self.output == "torch":
            return self._with_graph(self._obs(b.out.t))
        return self._with_graph(self._obs(b.to_host(self._obs_names)))

    def _need_cells(self, what):
        if not self.checkpoint_cells:
            raise RuntimeError("%s: this env was created without checkpoint_cells (no cell index)" % what)

    def archive_explore(self, score=None):
        """Go-Explore's archive update (checkpoint_cells=True): every env whose state is the best seen of its (level,
        switch_activated, 24 px cell) is stored in the cell's slot.  score [N] f32 (a CUDA tensor stays on the device), larger is
        better; None = the fewest frames to reach the cell.  Returns the status i32 [N]: 0 stored, 5 not eligible, 6 lost,
        7 archive full."""
        self._need_cells("archive_explore")
        return self._host(self._b.archive_explore(score=score, status=True))

    def archive_cells(self):
        """The cell index's tables (NppBatch.archive_cells): CUDA views [n_levels, 2, 25, 44], slot_key and n_used."""
        self._need_cells("archive_cells")
        return self._b.archive_cells()

    def restart_from_archive(self, mask):
        """Between two steps: every env whose mask byte is set restarts from a slot drawn among the occupied cells of its own
        level with weight 1 / sqrt(visits + chosen + 1) (an env whose level holds no cell is left alone) -- archive_select, then
        restart(): its observation dict, and its NotImplementedError with frame stacking / frame augmentation.  The slots used
        ([N] int32 CUDA tensor, -1 = none) are kept as last_restart_slots."""
        self._need_cells("restart_from_archive")
        self._restart_refusal()   # (before a draw is spent)
        self.last_restart_slots = self._b.archive_select(mask)
        return self.restart(self.last_restart_slots)

    def _level_of_map(self):
        """{map bytes: level id} of the env's level set (the first level of a map that comes twice); a level whose values are
        not bytes matches no replay."""
        if self._map_ids is None:
            self._map_ids = {}
            for k, m in enumerate(self._levels):
                if not isinstance(m, (bytes, bytearray)):
                    a = np.asarray(m, dtype=np.float64).ravel()
                    if not ((a >= 0) & (a <= 255) & (a == np.floor(a))).all():
                        continue
                    m = a.astype(np.uint8).tobytes()
                self._map_ids.setdefault(bytes(m), k)
        return self._map_ids

    def seed_archive_from_replays(self, replays, score="progress", max_demos_per_level=10):
        """Seed the cell index (checkpoint_cells=True) from expert demonstrations before training starts: the reference's
        DemoCheckpointSeeder (replay/demo_checkpoint_seeder.py), played as one batch with this env's own envs as players
        (NppBatch.archive_seed).  The state after every tick of every played replay is offered to the index as by
        archive_explore -- best score per (level, switch_activated, 24 px cell), no checkpoint within 72 px of the exit door once the
        switch is on -- but visits and chosen stay as they are: the seeder adds cells, not visits.  With record_routes, every seeded
        slot carries the actions that lead to it (frame_skip 1), so restart() leaves them as the env's own route.

        replays   CompactReplay objects or paths of .replay files.  Failures (success byte 0) are skipped, as load_demonstrations
                  skips them.  A replay is matched to the env's levels by its map bytes (the reference matches by file name,
                  demo_checkpoint_seeder.py:69-116); at most max_demos_per_level replays per level are kept, in the caller's order.
        score     "progress": tick / length, the seeder's score without a reward calculator (:777-779); "frames": archive_explore's
                  score=None, so that seeded cells are on the scale of cells found in training; or a list with one f32 array / tensor
                  of length L per replay (any return the trainer computed; NaN = not eligible; entries of replays that are not
                  played are ignored and may be None).
        Returns {"status": i32 [R] (0 played, 1 no level of this env has the map, 2 failure skipped, 3 over max_demos_per_level),
        "counts": i32 [R, 4] (candidates, eligible, stored, archive full per replay), "cells": n_used after the call}.
        Reward mode "pbrs" and action masking are switched off for the seeding and on again before the closing reset.  The call ends
        with the previous level assignment put back, whose own reset is a full reset of every env: the env is as the constructor
        left it, and reset() must follow before the next step().  Raises NotImplementedError, naming the option, with frame
        stacking, frame augmentation, level_weights or obs_overlap: their books advance per observation or per stream part, and a
        reset does not put them back."""
        self._need_cells("seed_archive_from_replays")
        for on, name in ((self._vk, "enable_visual_frame_stacking"), (self._sk, "enable_state_stacking"), (self._aug, "enable_augmentation"),
                         (self._pool, "level_weights"), (self._obs_overlap, "obs_overlap")):
            if on:
                raise NotImplementedError("seed_archive_from_replays with %s: the seeding plays outside its bookkeeping and a full "
                                          "reset does not restore it" % name)
        from .demos import _as_replay

        b = self._b
        reps = [_as_replay(r) for r in replays]
        table_mode = not isinstance(score, str)
        if table_mode and len(score) != len(reps):
            raise ValueError("seed_archive_from_replays: score must be \"progress\", \"frames\" or one array per replay")
        if not table_mode and score not in ("progress", "frames"):
            raise ValueError("seed_archive_from_replays: score must be \"progress\", \"frames\" or one array per replay, not %r" % (score,))
        status = np.zeros(len(reps), dtype=np.int32)
        ids, per_level, played, level_ids = self._level_of_map(), {}, [], []
        for i, r in enumerate(reps):
            if not r.success:
                status[i] = 2
            elif r.map_data not in ids:
                status[i] = 1
            elif per_level.get(ids[r.map_data], 0) >= int(max_demos_per_level):
                status[i] = 3
            else:
                per_level[ids[r.map_data]] = per_level.get(ids[r.map_data], 0) + 1
                played.append(i)
                level_ids.append(ids[r.map_data])
        counts = np.zeros((len(reps), 4), dtype=np.int32)
        if played:
            lengths = np.array([len(reps[i].input_sequence) for i in played], dtype=np.int64)
            offsets = np.zeros(len(played) + 1, dtype=np.int64)
            np.cumsum(lengths, out=offsets[1:])
            table = np.zeros(max(int(offsets[-1]), 1), dtype=np.uint8)
            for k, i in enumerate(played):
                table[offsets[k]:offsets[k + 1]] = np.asarray(reps[i].input_sequence, dtype=np.uint8)
            scores = None
            if table_mode:
                parts = []
                with b._ctx():
                    for k, i in enumerate(played):
                        s = score[i]
                        s = s.detach().to(device=b.device, dtype=torch.float32) if isinstance(s, torch.Tensor) else \
                            torch.from_numpy(np.ascontiguousarray(s, dtype=np.float32)).to(b.device)
                        if s.dim() != 1 or s.numel() != int(lengths[k]):
                            raise ValueError("seed_archive_from_replays: score[%d] must hold one value per tick (%d)" % (i, int(lengths[k])))
                        parts.append(s)
                    scores = torch.cat(parts) if int(offsets[-1]) else torch.zeros(1, dtype=torch.float32, device=b.device)
            before = b.env_levels()
            mask_mode = b._masking
            if mask_mode:
                b.set_action_masking(0)
            if self._pbrs:
                b.set_reward_mode("sparse")
            try:
                got = b.archive_seed(table, offsets, np.array(level_ids, dtype=np.int32), "table" if table_mode else score, scores=scores,
                                     counts=True)
            finally:
                if mask_mode:
                    b.set_action_masking(mask_mode)
                self._pbrs_on()
                b.assign_levels(before)   # (its own reset is Simulator.reset with fresh entities: the state the constructor left)
            with b._ctx():
                counts[played] = got.cpu().numpy()
        with b._ctx():
            cells = int(b.archive_cells()["n_used"].cpu()[0])
            out = {"status": status, "counts": counts, "cells": cells}
            if self.output == "torch":
                out["status"], out["counts"] = torch.from_numpy(status).to(b.device), torch.from_numpy(counts).to(b.device)
        return out

    # -- action routes -------------------------------------------------------------------------------
    def _need_routes(self, what):
        if not self.route_capacity:
            raise RuntimeError("%s: this env was created without record_routes (no action routes)" % what)

    def get_action_sequence_length(self):
        """[N] int32: the number of actions on every env's current route (base_environment.py:2341-2349, batched).  A device
        view for output="torch" (rewritten by the next step), a host copy for "numpy"."""
        self._need_routes("get_action_sequence_length")
        lens = self._b.route_views()[1][:, 0]
        if self.output == "torch":
            return lens
        self._b.join()
        with self._b._ctx():
            return lens.cpu().numpy()

    def get_current_action_sequence(self, env):
        """u8 array: the actions that led env `env` from its spawn to its current state (base_environment.py:2332-2339); after
        reset(options={"checkpoint": seq}) that is seq, after a restart from the archive the slot's route.  Synchronises."""
        self._need_routes("get_current_action_sequence")
        act, hdr = self._b.route_views()
        self._b.join()
        with self._b._ctx():
            h = hdr[int(env)].cpu().numpy()
            return act[int(env), int(h[12]), :int(h[0])].cpu().numpy()

    @staticmethod
    def _route_dict(hdr, actions):
        return {"actions": np.array(actions[:int(hdr[0])], dtype=np.uint8), "frame_count": int(hdr[3]), "level": int(hdr[5]),
                "frame_skip": int(hdr[2]), "bits": int(hdr[1])}

    def finished_routes(self, mask=None):
        """The route of the episode that ended last, for every env (or those with a non-zero mask byte) that has one: a list of
        dicts {"env", "actions" u8 array, "frame_count", "level", "frame_skip", "bits" (1 = actions were dropped at the capacity,
        2 = not replayable), "flags" (the flags byte of the episode's last step: 1 won, 2 dead, 8 truncated)} -- the keys of
        StateCheckpoint.get_compact_representation() the device knows.  The bytes stay valid on the device until the env's next
        episode ends.  Synchronises."""
        self._need_routes("finished_routes")
        act, hdr = self._b.route_views()
        self._b.join()
        with self._b._ctx():
            h = hdr.cpu().numpy()
            envs = np.flatnonzero((h[:, 6] > 0) | (h[:, 7] != 0))
            if mask is not None:
                m = mask.cpu().numpy() if isinstance(mask, torch.Tensor) else np.asarray(mask)
                envs = envs[m[envs] != 0]
            if not len(envs):
                return []
            idx = torch.from_numpy(envs).to(self._b.device)
            a = act[idx, torch.from_numpy(1 - h[envs, 12]).to(self._b.device).long()].cpu().numpy()
        out = []
        for k, e in enumerate(envs):
            d = self._route_dict(h[e, 6:12], a[k])
            d.update(env=int(e), flags=int(h[e, 10]))
            out.append(d)
        return out

    def archive_routes(self, slot_ids):
        """The routes of archive slots, for export: a list (one per slot id, None for an empty slot) of dicts with the keys of
        StateCheckpoint.get_compact_representation() the device knows -- "cell" (x, y) 24 px cell, "actions" u8 array,
        "frame_count", "position", "velocity", "switch" (from the archive's meta rows) -- and "slot", "level", "frame_skip",
        "bits".  Synchronises."""
        if not self.checkpoint_slots:
            raise RuntimeError("archive_routes: this env was created without checkpoint_slots (no checkpoint archive)")
        self._need_routes("archive_routes")
        slots = np.asarray(slot_ids.cpu() if isinstance(slot_ids, torch.Tensor) else slot_ids, dtype=np.int64).ravel()
        if len(slots) and (slots.min() < 0 or slots.max() >= self.checkpoint_slots):
            raise ValueError("archive_routes: slot ids must be in [0, checkpoint_slots)")
        act, hdr = self._b.archive_route_views()
        meta = self._b.archive_meta()
        self._b.join()
        with self._b._ctx():
            idx = torch.from_numpy(slots).to(self._b.device)
            h, a = hdr[idx].cpu().numpy(), act[idx].cpu().numpy()
            m = {k: v[idx].cpu().numpy() for k, v in meta.items()}
        out = []
        for k, s in enumerate(slots):
            if not m["stored"][k]:
                out.append(None)
                continue
            d = self._route_dict(h[k], a[k])
            d.update(slot=int(s), cell=(int(m["cell_x"][k]), int(m["cell_y"][k])), position=(float(m["x"][k]), float(m["y"][k])),
                     velocity=(float(m["vx"][k]), float(m["vy"][k])), switch=bool(m["switch_activated"][k]))
            out.append(d)
        return out

    def action_space_sample(self):
        """uint8 [N] uniform actions from the generator reset(seed=...) seeds."""
        return self._rng.integers(0, 6, size=self.num_envs).astype(np.uint8)

    def step_async(self, actions):
        """Enqueue the step (action upload, step kernel, observation kernels) on the handle's stream; returns at once."""
        b = self._b
        with b._ctx():
            if isinstance(actions, torch.Tensor):
                self._actions.copy_(actions.to(torch.uint8), non_blocking=True)
            else:
                self._actions.copy_(torch.as_tensor(np.asarray(actions, dtype=np.uint8)), non_blocking=True)
        b.step(self._actions, self.frame_skip, want_terminal=True)
        self._produce()
        if self._pbrs:
            # the reference's reward, into the block's reward.  Behind the observation kernels: the launch joins an observation
            # overlap, which has then done its work
            if self._waypoints:
                b.step_reward(wp_bonus_out=self._wp_bonus, wp_info_out=self._wp_info)
            else:
                b.step_reward()
        if self._episode:   # behind the reward launch: the block's flags, frames and reward rows, and in pbrs mode the components
            b.episode_accumulate(components=b.out.t["reward_components"] if self._pbrs else None, ended=self._ep_ended)

    def _episode_info(self):
        """info["_episode"] and info["episode"] of the step just accumulated"""
        v = self._b.episode_views()
        i32, f64, ended = v["i32"][6:14], v["f64"][7:14], self._ep_ended
        if self.output == "numpy":
            with self._b._ctx():   # (to_host has synchronised the stream the accumulation ran on)
                i32, f64, ended = i32.cpu().numpy(), f64.cpu().numpy(), ended.cpu().numpy()
        steps, frames, sw_step, sw_frames, level, bits, flags = (i32[k] for k in range(7))
        where = torch.where if self.output == "torch" else np.where
        ep = {"r": f64[0], "l": frames, "steps": steps, "is_success": (flags & 1) != 0, "switch_activated": sw_step != 0,
              "switch_activation_frame": where(sw_step != 0, sw_frames, -1 if self.output == "numpy" else torch.full_like(sw_frames, -1)),
              "level_id": level, "from_checkpoint": (bits & 2) != 0}
        if self._goal:   # the base level plus the stage the episode was played at (level -1: no episode yet)
            g = self._b.goal_views()
            base_of, stage_of = g["base_of"], g["stage_of"]
            if self.output == "torch":
                base_of, stage_of = (torch.from_numpy(t).to(self._b.device) for t in (base_of, stage_of))
                idx = level.clamp(min=0).long()
            else:
                idx = np.maximum(level, 0)
            ep["level_row"] = level
            ep["level_id"] = where(level >= 0, base_of[idx], -1 if self.output == "numpy" else torch.full_like(level, -1))
            ep["stage"] = where(level >= 0, stage_of[idx], -1 if self.output == "numpy" else torch.full_like(level, -1))
        if self._pbrs:
            ep["pbrs_total"], ep["terminal_reward"] = f64[1], f64[5]
        return ended != 0, ep

    def episode_level_stats(self):
        """episode_stats=True: {column: [L]} of the level table -- episodes, won, dead, truncated, dead_mine, dead_impact, switch,
        steps, frames, won_frames, return_fix (the returns' sum in units of 2^-20), restored, abandoned (int64) -- plus success_rate =
        won / episodes and mean_return (float64), both 0 where a level has no episode yet.  Episodes begun by a checkpoint count in
        `restored` alone."""
        if not self._episode:
            raise RuntimeError("episode_level_stats: this env was created without episode_stats")
        b = self._b
        with b._ctx():
            t = b.episode_level_table().clone()
            out = {name: t[:, k] for k, name in enumerate(b.EPISODE_COLUMNS)}
            n = out["episodes"].to(torch.float64)
            some = n > 0
            div = torch.where(some, n, torch.ones_like(n))
            out["success_rate"] = torch.where(some, out["won"].to(torch.float64) / div, torch.zeros_like(n))
            out["mean_return"] = torch.where(some, out["return_fix"].to(torch.float64) / 1048576.0 / div, torch.zeros_like(n))
            if self.output == "numpy":
                out = {k: v.cpu().numpy() for k, v in out.items()}
        return out

    def reset_episode_level_stats(self):
        if not self._episode:
            raise RuntimeError("reset_episode_level_stats: this env was created without episode_stats")
        self._b.episode_table_reset()

    # -- evaluation sweep (the reference's eval_mode, env_map_loader.py:138-162) ------------------------------
    def start_evaluation(self, levels=None, episodes_per_level=1):
        """Evaluate on a fixed list of levels (default: every loaded level), each played exactly episodes_per_level times: the job
        list is tile(levels, K), env e starts on job e and every env takes the next job when its episode ends; envs that find the
        list used up idle.  Returns (obs, info) like reset().  Needs episode_stats=True (the results are its records).  From here
        to stop_evaluation() step() adds info["evaluation"] = {"active": bool [N], "job": int32 [N]} and reset() is refused."""
        if not self._episode:
            raise RuntimeError("start_evaluation: this env was created without episode_stats=True, and an evaluation's results are "
                               "the episode records")
        K = int(episodes_per_level)
        if K < 1:
            raise ValueError("start_evaluation: episodes_per_level must be >= 1")
        lv = np.arange(len(self._levels), dtype=np.int32) if levels is None else np.asarray(levels, dtype=np.int32).ravel()
        if len(lv) == 0:
            raise ValueError("start_evaluation: no levels")
        self._b.sweep_start(np.tile(lv, K))
        self._sweep = self._swept = True
        self._eval = {"levels": lv.copy(), "episodes_per_level": K}
        return self._reset_return({"evaluation": {"levels": lv.copy(), "episodes_per_level": K, "jobs": len(lv) * K}})

    def stop_evaluation(self):
        """End the evaluation (finished or not): every env keeps the level it plays; evaluation_results() stays readable."""
        self._b.sweep_stop()
        self._sweep = False

    def _need_evaluation(self, what):
        if getattr(self, "_eval", None) is None:
            raise RuntimeError("%s: no evaluation was started (start_evaluation)" % what)
        return self._b.sweep_state()

    def evaluation_done(self):
        """True once every job has finished.  One 12-byte read that synchronises: call it every few steps, not every step."""
        s = self._need_evaluation("evaluation_done")
        with self._b._ctx():
            c = s["counters"].cpu().numpy()
        return int(c[1]) == int(c[2])

    def evaluation_results(self):
        """The outcome of every job, in job order (job j = episode j // L of level levels[j % L]): {"level", "env" (-1: not
        played yet), "done", "is_success", "dead", "truncated", "death_cause", "steps", "frames", "switch_frames" (-1: the switch was
        never activated), "r"} (+ "pbrs_components" [J, 6] with reward_mode="pbrs"), each [J], and "per_level" = {"level",
        "episodes", "success_rate", "mean_return", "mean_frames"} [L], reduced in float64 over the [K, L] reshape along axis 0, so
        the same results give the same bits.  Synchronises."""
        s = self._need_evaluation("evaluation_results")
        with self._b._ctx():
            i32, f64 = s["i32"].cpu().numpy(), s["f64"].cpu().numpy()
        steps, frames, sw_step, sw_frames, _level, _bits, flags, env, status = i32
        out = {"level": s["jobs"].copy(), "env": env, "done": status != 0, "is_success": (flags & 1) != 0, "dead": (flags & 2) != 0,
               "truncated": (flags & 8) != 0, "death_cause": (flags >> 4) & 3, "steps": steps, "frames": frames,
               "switch_frames": np.where(sw_step != 0, sw_frames, -1), "r": f64[0]}
        if self._pbrs:
            out["pbrs_components"] = np.ascontiguousarray(f64[1:7].T)
        per = reduce_evaluation(self._eval["levels"], self._eval["episodes_per_level"], out["done"], out["is_success"], out["r"], frames)
        if self.output == "torch":
            with self._b._ctx():
                out = {k: torch.from_numpy(np.ascontiguousarray(v)).to(self._b.device) for k, v in out.items()}
                per = {k: torch.from_numpy(v).to(self._b.device) for k, v in per.items()}
        out["per_level"] = per
        return out

    def evaluate(self, policy, levels=None, episodes_per_level=1, max_steps=None, check_every=16):
        """start_evaluation(), then step with actions = policy(obs) until every job has finished (looked at every check_every steps)
        or max_steps steps have run, then stop_evaluation().  Returns evaluation_results(); jobs that did not finish have done False."""
        obs, _ = self.start_evaluation(levels, episodes_per_level)
        try:
            t = 0
            while max_steps is None or t < int(max_steps):
                obs = self.step(policy(obs))[0]
                t += 1
                if t % int(check_every) == 0 and self.evaluation_done():
                    break
            return self.evaluation_results()
        finally:
            self.stop_evaluation()

    def step_wait(self):
        """Results of the step enqueued by step_async: (obs, reward, terminated, truncated, info) with batch dims.
        output="torch": device tensors, no synchronisation (consume them on the handle's stream);
        output="numpy": ONE async copy of the output block into pinned memory + one synchronisation."""
        b = self._b
        if self.output == "torch":
            src = self._stacked(b.out.t, with_terminal=True)
        else:
            stk = self._stacked({}, with_terminal=True)   # (copies enqueued before to_host's synchronisation)
            src = b.to_host(self._obs_names + ["reward", "frames", "terminal_state"] + (["reward_components"] if self._pbrs else []))
            src.update(stk)
        flags = src["flags"]
        info = {
            "player_won": (flags & 1) != 0,
            "player_dead": (flags & 2) != 0,
            "switch_activated": (flags & 4) != 0,
            "death_cause_code": (flags >> 4) & 3,
            "frames_executed": src["frames"],
            "terminal_observation": src["terminal_state"],
            "frame_skip_stats": {"skip_value": self.frame_skip},
        }
        if "terminal_game_state_stack" in src:
            info["terminal_game_state_stack"] = src["terminal_game_state_stack"]
        info["level_id"] = raw_levels = self._level_id(self.output == "numpy")
        if self._goal:   # the base level plus the stage; the rows of the level set (variants included) stay in info["level_row"]
            base, info["goal_curriculum"] = self._goal_info(raw_levels)
            info["level_row"] = raw_levels
            info["level_id"] = base if self.output == "numpy" else torch.from_numpy(base).to(self._b.device)
        if self._mask_on:
            info.update(self._mask_info(src, (flags & 11) != 0))
        if self._pbrs:
            info["pbrs_components"] = src["reward_components"]
        if self._waypoints:   # the step's unscaled bonus, the collected sequence index or -1, the next expected index, the collected count
            wb, wi = self._wp_bonus, self._wp_info
            if self.output == "numpy":
                with b._ctx():   # (to_host above has synchronised the stream the reward launches ran on)
                    wb, wi = wb.cpu().numpy(), wi.cpu().numpy()
            info["waypoints"] = {"bonus": wb, "index": wi[:, 0], "next_expected": wi[:, 1], "collected": wi[:, 2]}
        if self._episode:
            info["_episode"], info["episode"] = self._episode_info()
        if self._sweep:   # the job every env plays from this observation on (-1: idle, the list is used up)
            job = b.sweep_state()["env_job"]
            if self.output == "numpy":
                with b._ctx():
                    job = job.cpu().numpy()
            else:
                job = job.clone()
            info["evaluation"] = {"active": job >= 0, "job": job}
        return self._with_graph(self._obs(src), raw_levels), src["reward"], (flags & 3) != 0, (flags & 8) != 0, info

    def step(self, actions):
        """actions: int array/tensor [N] in 0..5.  Returns (obs, reward, terminated, truncated, info) with batch dims."""
        self.step_async(actions)
        return self.step_wait()

    def close(self):
        self._b.close()

    @property
    def batch(self):
        return self._b


class _HostGraphRows:
    """output="numpy" graph observations: the device's changed-rows rule on the host.  Two buffer sets alternate (the previous
    observation's arrays stay valid); each records the level its rows hold and rewrites, whole, the rows of envs whose level
    differs.  The per-level rows come from npp_graph_compile, built the first time a level is needed."""

    def __init__(self, levels, n):
        self._blob, self._off = _as_f64_blob(levels)
        self._n = n
        self._tabs = {}
        self._sets = [None, None]
        self._next = 0

    def _table(self, level):
        t = self._tabs.get(level)
        if t is None:
            feats, edges, nn, ne = graph_tables(self._blob[self._off[level]:self._off[level + 1]])
            t = self._tabs[level] = {"graph_node_feats": feats, "graph_edge_index": edges,
                                     "graph_node_mask": (np.arange(2500) < nn).astype(np.uint8),
                                     "graph_edge_mask": (np.arange(20000) < ne).astype(np.uint8)}
        return t

    def update(self, levels):
        levels = np.asarray(levels, dtype=np.int32)
        k = self._next
        self._next ^= 1
        if self._sets[k] is None:
            np_dtype = {torch.float32: np.float32, torch.uint16: np.uint16, torch.uint8: np.uint8}
            bufs = {name: np.zeros((self._n,) + shape, dtype=np_dtype[dt]) for name, (shape, dt) in GRAPH_KEYS.items()}
            self._sets[k] = (bufs, np.full(self._n, -1, dtype=np.int32))
        bufs, held = self._sets[k]
        changed = np.flatnonzero(held != levels)
        for level in np.unique(levels[changed]):
            envs = changed[levels[changed] == level]
            for name, row in self._table(int(level)).items():
                bufs[name][envs] = row
            held[envs] = level
        return dict(bufs)


class NppEnvironment:
    """Single-environment adapter with the reference's exact call signatures (base_environment.py:483,
    npp_environment.py:504).  One GPU lane group does the work of one Python simulator; use NppVecEnvironment for
    throughput.  Frame stacking takes NppVecEnvironment's arguments; stacked keys come without the batch dimension
    (player_frame (K, 84, 84, 1), game_state (K, 41)).  observation_mode="minimal": NppVecEnvironment's minimal mode
    (minimal_observation (40,), action_mask (6,) and the pass-through scalars; no terminal minimal observation).
    enable_augmentation / augmentation_p / augmentation_intensity / augmentation_seed: NppVecEnvironment's frame augmentation.
    checkpoint_slots / archive_store(slot) / reset(options={"checkpoint": {"slots": [slot]}}): NppVecEnvironment's checkpoint archive;
    checkpoint_cells / checkpoint_seed are passed through to it.
    action_masking_mode / set_action_masking_mode(mode): NppVecEnvironment's path-direction action masking; info["path_direction"] is
    an int, and the step that ends the episode adds info["deterministic_mask_applied_count"] / info["deterministic_mask_rate"].
    reward_mode / reward_params / set_reward_params(**kw): NppVecEnvironment's reward mode "pbrs"; info["pbrs_components"] is (6,).
    goal_curriculum=True / goal_curriculum_params / set_curriculum_stage(stage) / goal_curriculum_state(): NppVecEnvironment's goal
    curriculum.  This class never auto-resets and the curriculum's counters are kept behind auto-resetting steps only,
    so info["goal_curriculum"]'s three counters stay 0 and the stage moves only through set_curriculum_stage.
    episode_stats=True: the step that ends the episode adds the reference's info["r"] (the return), info["l"] (frames),
    info["is_success"] and info["switch_activation_frame"] (base_environment.py:1163-1242; NppVecEnvironment's episode statistics)."""

    def __init__(self, map_data=None, custom_map_path=None, frame_skip=4, device=0, enable_visual_observations=False,
                 truncation_limit="dynamic", fast_reset=True, enable_spatial_context=False, enable_switch_states=False,
                 enable_reachability=False, enable_visual_frame_stacking=False, visual_stack_size=4, enable_state_stacking=False,
                 state_stack_size=4, frame_stack_padding_type="zero", enable_graph_observations=False, observation_mode="full",
                 enable_augmentation=False, augmentation_p=0.5, augmentation_intensity="medium", augmentation_seed=None,
                 checkpoint_slots=0, checkpoint_cells=False, checkpoint_seed=0, record_routes=False, route_capacity=None,
                 action_masking_mode=None, reward_mode="sparse", reward_params=None, reward_waypoints=False, waypoint_params=None,
                 episode_stats=False, goal_curriculum=False, goal_curriculum_params=None):
        spaces.check_frame_augmentation(augmentation_p, augmentation_intensity)
        spaces.check_observation_mode(
            observation_mode, enable_visual_observations=enable_visual_observations,
            enable_visual_frame_stacking=enable_visual_frame_stacking, enable_state_stacking=enable_state_stacking,
            enable_graph_observations=enable_graph_observations, enable_spatial_context=enable_spatial_context,
            enable_reachability=enable_reachability, enable_switch_states=enable_switch_states,
            enable_augmentation=enable_augmentation)
        if map_data is None:
            if custom_map_path is None:
                raise ValueError("NppEnvironment needs map_data or custom_map_path")
            with open(custom_map_path, "rb") as f:
                map_data = np.frombuffer(f.read(), dtype=np.uint8)
        self._v = NppVecEnvironment([map_data], 1, level_ids=[0], frame_skip=frame_skip, device=device,
                                    enable_visual_observations=enable_visual_observations,
                                    truncation_limit=truncation_limit, output="numpy", autoreset=False,
                                    fast_reset=fast_reset, enable_spatial_context=enable_spatial_context,
                                    enable_switch_states=enable_switch_states, enable_reachability=enable_reachability,
                                    enable_visual_frame_stacking=enable_visual_frame_stacking, visual_stack_size=visual_stack_size,
                                    enable_state_stacking=enable_state_stacking, state_stack_size=state_stack_size,
                                    frame_stack_padding_type=frame_stack_padding_type,
                                    enable_graph_observations=enable_graph_observations, observation_mode=observation_mode,
                                    enable_augmentation=enable_augmentation, augmentation_p=augmentation_p,
                                    augmentation_intensity=augmentation_intensity, augmentation_seed=augmentation_seed,
                                    checkpoint_slots=checkpoint_slots, checkpoint_cells=checkpoint_cells,
                                    checkpoint_seed=checkpoint_seed, record_routes=record_routes, route_capacity=route_capacity,
                                    action_masking_mode=action_masking_mode, reward_mode=reward_mode, reward_params=reward_params,
                                    reward_waypoints=reward_waypoints, waypoint_params=waypoint_params, episode_stats=episode_stats,
                                    goal_curriculum=goal_curriculum, goal_curriculum_params=goal_curriculum_params)
        self.action_space = self._v.single_action_space
        self.observation_space = self._v.single_observation_space
        self.frame_skip = frame_skip

    def set_curriculum_stage(self, stage):
        """goal_curriculum=True: the stage from the next reset on (the reference's method, base_environment.py:404-481)"""
        self._v.set_curriculum_stage(stage, 0)

    def goal_curriculum_state(self):
        return self._v.goal_curriculum_state()

    @staticmethod
    def _unbatch(obs):
        out = {k: v[0].copy() if isinstance(v[0], np.ndarray) else v[0] for k, v in obs.items()}
        for k in ("player_x", "player_y", "switch_x", "switch_y", "exit_door_x", "exit_door_y"):
            out[k] = float(out[k])
        for k in ("switch_activated", "player_won", "player_dead"):   # (the last two: minimal mode)
            if k in out:
                out[k] = bool(out[k])
        if "death_cause" in out:
            out["death_cause"] = int(out["death_cause"])
        return out

    def reset(self, seed=None, options=None):
        obs, info = self._v.reset(seed=seed, options=options)
        if "path_direction" in info:
            info["path_direction"] = int(info["path_direction"][0])
        return self._unbatch(obs), info

    def set_action_masking_mode(self, mode):
        self._v.set_action_masking_mode(mode)

    def set_reward_params(self, **kw):
        self._v.set_reward_params(**kw)

    def set_waypoint_params(self, **kw):
        self._v.set_waypoint_params(**kw)

    def level_waypoints(self, level):
        return self._v.level_waypoints(level)

    def archive_store(self, slot):
        """Store the current state in slot `slot` of the checkpoint archive (checkpoint_slots > 0); returns the status (0 =
        stored).  reset(options={"checkpoint": {"slots": [slot]}}) restarts from it."""
        return int(self._v.archive_store(np.array([int(slot)], dtype=np.int32))[0])

    def get_current_action_sequence(self):
        """The actions taken since the last reset, as a list of ints (base_environment.py:2332-2339); record_routes=True."""
        return [int(a) for a in self._v.get_current_action_sequence(0)]

    def get_action_sequence_length(self):
        """len(get_current_action_sequence()) without the copy of the bytes (base_environment.py:2341-2349)."""
        return int(self._v.get_action_sequence_length()[0])

    def step(self, action):
        obs, rew, term, trunc, info = self._v.step(np.array([int(action)], dtype=np.uint8))
        cause = DEATH_CAUSES[int(info["death_cause_code"][0])]
        out_info = {
            "player_won": bool(info["player_won"][0]),
            "player_dead": bool(info["player_dead"][0]),
            "switch_activated": bool(info["switch_activated"][0]),
            "death_cause": cause,
            "frame_skip_stats": {"skip_value": self.frame_skip, "frames_executed": int(info["frames_executed"][0])},
        }
        if "path_direction" in info:
            out_info["path_direction"] = int(info["path_direction"][0])
            if bool(term[0]) or bool(trunc[0]):
                out_info["deterministic_mask_applied_count"] = int(info["deterministic_mask_applied_count"][0])
                out_info["deterministic_mask_rate"] = float(info["deterministic_mask_rate"][0])
        if "pbrs_components" in info:
            out_info["pbrs_components"] = np.array(info["pbrs_components"][0], dtype=np.float32)
        if "waypoints" in info:
            w = info["waypoints"]
            out_info["waypoints"] = {"bonus": float(w["bonus"][0]), "index": int(w["index"][0]), "next_expected": int(w["next_expected"][0]),
                                     "collected": int(w["collected"][0])}
        if "goal_curriculum" in info:   # get_curriculum_info's fields of this env (positions as (x, y) tuples)
            gc = info["goal_curriculum"]
            out_info["goal_curriculum"] = {k: (v if np.isscalar(v) else (tuple(float(x) for x in v[0]) if np.ndim(v) == 2 else v[0].item()))
                                           for k, v in gc.items()}
        if "_episode" in info and bool(info["_episode"][0]):
            ep = info["episode"]
            out_info.update({"r": float(ep["r"][0]), "l": int(ep["l"][0]), "is_success": bool(ep["is_success"][0]),
                             "switch_activation_frame": int(ep["switch_activation_frame"][0])})
        return self._unbatch(obs), float(rew[0]), bool(term[0]), bool(trunc[0]), out_info

    def close(self):
        self._v.close()


class _SimView:
    """`.sim.frame` of the facade."""

    def __init__(self, owner):
        self._o = owner

    @property
    def frame(self):
        return int(self._o._state()[1][0, 22])


class NPlayHeadless:
    """The reference's headless facade for one simulator, backed by the GPU stepper (nplay_headless.py:28).

    Method names, argument meaning and return conventions follow the reference so that harnesses such as
    tools/test_replay_playback.py read the same."""

    def __init__(self, device=0, enable_rendering=False, **_ignored):
        self._device = device
        self._b = None
        self.sim = _SimView(self)
        self.current_map_data = None

    def load_map_from_map_data(self, map_data):
        if self._b is not None:
            self._b.close()
        self._b = NppBatch(1, device=self._device, autoreset=False, outputs=("positions",))
        self._b.load_levels([map_data])
        with self._b._ctx():
            self._in = torch.zeros((1, 1), dtype=torch.uint8, device=self._b.device)
        self.current_map_data = map_data
        self._cache = {}

    def load_map(self, map_path):
        with open(map_path, "rb") as f:
            self.load_map_from_map_data(np.frombuffer(f.read(), dtype=np.uint8))

    def reset(self):
        """Simulator.reset (nsim.py:62-76): entities re-created."""
        self._b.reset(mode="full")
        self._cache = {}

    def fast_reset(self):
        """Simulator.fast_reset (nsim.py:78-140): entities reset in place (key-ordered cell lists, movers keep going)."""
        self._b.reset(mode="fast")
        self._cache = {}

    def tick(self, horizontal_input, jump_input):
        with self._b._ctx():
            self._in.fill_(controls_to_input_byte(horizontal_input, jump_input))
        self._b.tick(self._in)
        self._cache = {}

    # accessors share ONE state dump / ONE observation per tick (they used to cost a device round trip each)
    def _state(self):
        if "state" not in self._cache:
            self._cache["state"] = self._b.dump_state(0, 1)
        return self._cache["state"]

    def _observed(self):
        if "obs" not in self._cache:
            self._b.observe()
            self._cache["obs"] = self._b.to_host(["game_state", "action_mask", "entity_pos", "positions"])
        return self._cache["obs"]

    def ninja_has_won(self):
        return int(self._state()[1][0, 0]) == 8

    def ninja_has_died(self):
        return int(self._state()[1][0, 0]) in (6, 7)

    def ninja_death_cause(self):
        return DEATH_CAUSES[int(self._state()[1][0, 20])]

    def ninja_position(self):
        f = self._state()[0][0]
        return float(f[0]), float(f[1])

    def ninja_velocity(self):
        f = self._state()[0][0]
        return float(f[2]), float(f[3])

    def ninja_velocity_old(self):
        f = self._state()[0][0]
        return float(f[8]), float(f[9])

    def get_ninja_terminal_impact(self):
        return bool(self._state()[1][0, 21])

    def get_ninja_state(self):
        return [float(v) for v in self._observed()["game_state"][0, :40]]

    def get_action_mask(self):
        return [bool(v) for v in self._observed()["action_mask"][0]]

    def exit_switch_activated(self):
        return int(self._state()[1][0, 13]) != 1

    def exit_switch_position(self):
        p = self._observed()["positions"][0]
        return float(p[2]), float(p[3])

    def exit_door_position(self):
        p = self._observed()["positions"][0]
        return float(p[4]), float(p[5])

    def render(self):
        """The gray frame, numpy uint8 (600, 1056, 1), as the reference's render() returns it (nplay_headless.py:144-156)."""
        return self._b.render_frame(0, 1)[0].cpu().numpy()

    def _entities(self):
        """(compiled rows [kind, x, y, cx, cy, init], live 2-bit states) of the loaded level, map order."""
        from .engine import compile_level_entities

        return compile_level_entities(self.current_map_data), self._b.dump_entities(0)

    def locked_doors(self):
        """Locked-door entities (entity_dic[6]) as simple records: the entity sits at its switch (xpos, ypos == sw_xpos,
        sw_ypos), `active` until the switch is collected, `closed` likewise (nplay_headless.py:714-716)."""
        from types import SimpleNamespace

        rows, st = self._entities()
        return [SimpleNamespace(type=6, xpos=float(r[1]), ypos=float(r[2]), sw_xpos=float(r[1]), sw_ypos=float(r[2]),
                                active=bool(st[i] & 1), closed=bool(st[i] & 1))
                for i, r in enumerate(rows) if int(r[0]) == 6]

    def get_mine_entities(self):
        """(toggle mines of type 1, of type 21) with xpos, ypos, state (0 toggled / deadly, 1 untoggled, 2 toggling)."""
        from types import SimpleNamespace

        rows, st = self._entities()
        m1, m21 = [], []
        for i, r in enumerate(rows):
            if int(r[0]) == 1:
                (m1 if int(r[5]) == 0 else m21).append(SimpleNamespace(xpos=float(r[1]), ypos=float(r[2]), state=int(st[i]), active=True))
        return m1, m21

    def exit(self):
        if self._b is not None:
            self._b.close()
            self._b = None
