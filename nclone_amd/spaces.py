"""Observation/action space descriptions.

Uses gymnasium's spaces when gymnasium is importable (so `isinstance` checks in training code work); otherwise
falls back to tiny stand-ins with the same attribute names (`n`, `shape`, `dtype`, `low`, `high`, `spaces`).
Shapes/dtypes follow the reference: nclone/gym_environment/base_environment.py:150,320-364.
"""
import numpy as np

try:  # pragma: no cover - gymnasium is not installed in the build container
    from gymnasium.spaces import Box, Dict, Discrete  # type: ignore
except Exception:  # noqa: BLE001

    class Discrete:  # type: ignore
        def __init__(self, n):
            self.n = int(n)
            self.shape = ()
            self.dtype = np.int64

        def sample(self, rng=None):
            rng = rng or np.random.default_rng()
            return int(rng.integers(0, self.n))

        def contains(self, x):
            return 0 <= int(x) < self.n

        def __repr__(self):
            return "Discrete(%d)" % self.n

    class Box:  # type: ignore
        def __init__(self, low, high, shape, dtype):
            self.low, self.high, self.shape, self.dtype = low, high, tuple(shape), np.dtype(dtype)

        def __repr__(self):
            return "Box(%r, %r, %r, %s)" % (self.low, self.high, self.shape, self.dtype)

    class Dict:  # type: ignore
        def __init__(self, spaces):
            self.spaces = dict(spaces)

        def __getitem__(self, k):
            return self.spaces[k]

        def keys(self):
            return self.spaces.keys()

        def __repr__(self):
            return "Dict(%r)" % self.spaces


def action_space():
    # 0 NOOP, 1 LEFT, 2 RIGHT, 3 JUMP, 4 JUMP+LEFT, 5 JUMP+RIGHT (base_environment.py:366-402)
    return Discrete(6)


def check_frame_stack(visual_stack_size=4, state_stack_size=4, padding_type="zero"):
    """The reference's argument checks, messages included (frame_stack_wrapper.py:116-121); both sizes are checked whether or
    not that key is stacked, as there."""
    if visual_stack_size < 1 or visual_stack_size > 12:
        raise ValueError("visual_stack_size must be between 1 and 12")
    if state_stack_size < 1 or state_stack_size > 12:
        raise ValueError("state_stack_size must be between 1 and 12")
    if padding_type not in ["zero", "repeat"]:
        raise ValueError("padding_type must be 'zero' or 'repeat'")


def check_frame_augmentation(p=0.5, intensity="medium"):
    """The reference's argument checks, messages included (AugmentationConfig.__post_init__, config.py:82-87)."""
    if intensity not in ["light", "medium", "strong"]:
        raise ValueError("intensity must be one of ['light', 'medium', 'strong']")
    if not 0.0 <= p <= 1.0:
        raise ValueError("p must be between 0.0 and 1.0")


OBSERVATION_MODES = ("full", "minimal")   # gym_environment/config.py:17-20 ObservationMode


def check_observation_mode(observation_mode, **options):
    """The observation_mode argument of the host classes: "full" or "minimal" (anything else raises ValueError), and in minimal
    mode every option that is switched on although it has nothing to act on there -- `options` maps the constructor's names
    (enable_visual_observations, enable_state_stacking, ...) to their values -- raises ValueError naming the conflict.  Needs no
    device.  Returns True for minimal mode."""
    if observation_mode not in OBSERVATION_MODES:
        raise ValueError("observation_mode must be 'full' or 'minimal', not %r" % (observation_mode,))
    if observation_mode == "full":
        return False
    on = [k for k, v in options.items() if v]
    if on:
        raise ValueError("observation_mode='minimal' conflicts with %s: the minimal observation is minimal_observation (40 floats) and "
                         "action_mask only, so that option has nothing to act on" % ", ".join(on))
    return True


def observation_space(visual=False, spatial_context=False, switch_states=False, reachability=False, visual_stack=0, state_stack=0,
                      graph=False, minimal=False):
    """minimal: the reference's two-key Dict of its MINIMAL observation mode (npp_environment.py:211-231), whatever the other
    arguments say.  visual_stack / state_stack: K > 0 stacks player_frame to (K, 84, 84, 1) / game_state to (K, 41) with the bounds of the
    reference's stacked space (frame_stack_wrapper.py:139-181); global_view and the other keys pass through.  graph: the four
    graph observation keys (npp_environment.py:245-271)."""
    if minimal:
        return Dict({"minimal_observation": Box(-1.0, 1.0, (40,), np.float32), "action_mask": Box(0, 1, (6,), np.int8)})
    spaces = {
        "game_state": Box(-1.0, 1.0, (state_stack, 41) if state_stack else (41,), np.float32),
        "action_mask": Box(0, 1, (6,), np.int8),
        "entity_positions": Box(0.0, 1.0, (6,), np.float32),
    }
    if spatial_context:
        spaces["spatial_context"] = Box(-1.0, 1.0, (112,), np.float32)
    if switch_states:
        spaces["switch_states"] = Box(0.0, 1.0, (25,), np.float32)
    if visual:
        spaces["player_frame"] = Box(0, 255, (visual_stack, 84, 84, 1) if visual_stack else (84, 84, 1), np.uint8)
        spaces["global_view"] = Box(0, 255, (176, 100, 1), np.uint8)   # RENDERED_VIEW_HEIGHT x WIDTH (constants.py:18-19)
    if reachability:   # npp_environment.py observation space: reachability_features (38), mine_sdf_features (3)
        spaces["reachability_features"] = Box(0.0, 1.0, (38,), np.float32)   # the reference declares [0, 1] (npp_environment.py:236)
        spaces["mine_sdf_features"] = Box(-1.0, 1.0, (3,), np.float32)
    if graph:   # N_MAX_NODES = 2500, NODE_FEATURE_DIM = 6, E_MAX_EDGES = 20000 (graph/common.py:42-58)
        spaces["graph_node_feats"] = Box(-np.inf, np.inf, (2500, 6), np.float32)
        spaces["graph_edge_index"] = Box(0, 2499, (2, 20000), np.uint16)
        spaces["graph_node_mask"] = Box(0, 1, (2500,), np.uint8)
        spaces["graph_edge_mask"] = Box(0, 1, (20000,), np.uint8)
    return Dict(spaces)
