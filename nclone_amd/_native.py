"""ctypes binding of libnpp_amd.so (the C ABI in include/npp_amd.h).

There is NO CPU fallback: if the library is missing this module raises, and if no GPU is present
`npp_create` fails with a clear message.  The oracle under oracle/ is test infrastructure and is never
imported from here.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# NPP_AMD_LIB selects another build of the same library (tools/ab_bench.py-style A/B runs of kernel variants)
LIB_PATH = os.environ.get("NPP_AMD_LIB") or os.path.join(_HERE, "libnpp_amd.so")

NPP_OK = 0
NPP_ERR_INVALID, NPP_ERR_HIP, NPP_ERR_UNSUPPORTED, NPP_ERR_STATE = 1, 2, 3, 4
FLAG_AUTORESET = 1
FLAG_ALLOW_UNSUPPORTED = 2
FLAG_FRAME_CENTERED = 4
FLAG_FAST_RESET = 8
F_WON, F_DEAD, F_SWITCH, F_TRUNCATED, F_CAUSE_MINE, F_CAUSE_IMPACT = 1, 2, 4, 8, 16, 32
GAME_STATE_DIM = 41
MINIMAL_OBS_DIM = 40
DUMP_F64 = 12
DUMP_I32 = 32

EXPORTS = [
    "npp_create", "npp_destroy", "npp_last_error", "npp_set_stream", "npp_sync", "npp_load_levels",
    "npp_assign_levels", "npp_reset", "npp_set_truncation_limit", "npp_step", "npp_tick", "npp_observe",
    "npp_render_player_frame", "npp_dump_state", "npp_set_ninja_state", "npp_set_mover_state", "npp_dump_movers", "npp_state_decode_host", "npp_dump_entities", "npp_dump_level_segments",
    "npp_compile_level_segments", "npp_compile_level_entities", "npp_set_step_variant", "npp_get_step_variant", "npp_num_envs", "npp_num_levels",
    "npp_set_launch_geometry", "npp_get_launch_geometry", "npp_snapshot", "npp_restore", "npp_entity_checksum", "npp_compile_level_zoo", "npp_render_global_view", "npp_switch_states", "npp_set_entity_pos", "npp_step_many", "npp_render_frame", "npp_plan_zoo_block", "npp_reset_ex",
    "npp_reachability", "npp_reachability_ex", "npp_reach_compile", "npp_reach_features_host", "npp_reach_compile_miss", "npp_reach_rollout_host", "npp_set_dynamic_truncation", "npp_level_truncation_limit",
    "npp_set_obs_overlap", "npp_set_obs_overlap_parts", "npp_join",
    "npp_set_frame_stack", "npp_frame_stack_render", "npp_frame_stack_push", "npp_frame_stack_view",
    "npp_set_level_pool", "npp_draw_levels", "npp_get_env_levels", "npp_env_level_view", "npp_level_pool_draw_host",
    "npp_graph_observation", "npp_graph_compile",
    "npp_set_minimal_observation", "npp_minimal_observation", "npp_minimal_encode_host",
    "npp_set_frame_augmentation", "npp_frame_augment", "npp_frame_augment_view", "npp_frame_augment_params_host",
    "npp_frame_augment_apply_host",
    "npp_archive_create", "npp_archive_store", "npp_archive_restore", "npp_archive_meta_view", "npp_archive_num_slots",
    "npp_archive_record_bytes",
    "npp_archive_cells_create", "npp_archive_explore", "npp_archive_select", "npp_archive_cells_view",
    "npp_archive_cell_keys_host", "npp_archive_cell_pick_host",
    "npp_set_routes", "npp_route_view", "npp_archive_route_view", "npp_route_apply_host",
    "npp_set_action_masking", "npp_path_action_mask", "npp_path_mask_stats_view", "npp_path_direction_host",
    "npp_set_reward_mode", "npp_set_reward_params", "npp_step_reward", "npp_reward_default_params", "npp_reward_level_constants_host",
    "npp_reward_host",
    "npp_set_reward_waypoints", "npp_set_waypoint_params", "npp_step_reward_wp", "npp_reward_waypoints", "npp_waypoint_default_params",
    "npp_reward_waypoints_host", "npp_waypoint_bonus_host", "npp_reward_host_wp",
    "npp_demo_plan_host", "npp_demo_create", "npp_demo_destroy", "npp_demo_rows", "npp_demo_play",
    "npp_archive_seed", "npp_archive_seed_rows_host",
    "npp_set_episode_stats", "npp_episode_accumulate", "npp_episode_restart", "npp_episode_view", "npp_episode_table_reset",
    "npp_episode_apply_host",
    "npp_goal_default_params", "npp_set_goal_curriculum", "npp_goal_set_stage", "npp_goal_view", "npp_goal_tables", "npp_goal_stage_positions",
    "npp_goal_stages_host", "npp_goal_apply_host", "npp_compile_level_segments_goal", "npp_compile_level_entities_goal",
    "npp_reach_rollout_goal_host", "npp_path_direction_goal_host", "npp_reward_level_constants_goal_host", "npp_reward_goal_host",
    "npp_sweep_start", "npp_sweep_stop", "npp_sweep_view", "npp_sweep_assign_host",
]


class StepOut(C.Structure):
    _fields_ = [
        ("d_game_state", C.c_void_p),
        ("d_action_mask", C.c_void_p),
        ("d_entity_pos", C.c_void_p),
        ("d_flags", C.c_void_p),
        ("d_reward", C.c_void_p),
        ("d_frames", C.c_void_p),
        ("d_terminal_state", C.c_void_p),
        ("d_spatial_context", C.c_void_p),
        ("d_positions", C.c_void_p),
        ("d_work", C.c_void_p),
    ]


class GoalCurriculumParams(C.Structure):
    _fields_ = [("stage_distance_interval", C.c_double), ("advancement_threshold", C.c_double), ("rolling_window", C.c_int32),
                ("auto_advance", C.c_int32)]


class DemoOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in (
        "d_game_state", "d_action_mask", "d_entity_positions", "d_spatial_context", "d_reachability_features", "d_mine_sdf_features",
        "d_switch_states", "d_positions", "d_action", "d_frame", "d_done", "d_replay", "d_level", "d_flags", "d_status")]


DEMO_KEY_FLAGS = {"game_state": 1, "action_mask": 2, "entity_positions": 4, "spatial_context": 8, "reachability_features": 16,
                  "mine_sdf_features": 32, "switch_states": 64, "positions": 128}
DEMO_MASK_ENV = 1 << 16


class NativeLibraryMissing(RuntimeError):
    pass


_lib = None


def lib():
    """Load (once) and return the native library; raise loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own HIP runtime (torch/lib/libamdhip64.so) and publishes its symbols globally; it must be
    # loaded BEFORE this library so that both share ONE runtime (streams and device pointers are exchanged).
    import torch  # noqa: F401

    if not os.path.isfile(LIB_PATH):
        raise NativeLibraryMissing(
            "nclone_amd: %s not found. Build it with `python -m nclone_amd.build_native` (needs hipcc). "
            "There is no CPU fallback for the accelerated path." % LIB_PATH
        )
    L = C.CDLL(LIB_PATH)
    H = C.c_void_p
    L.npp_create.argtypes = [C.c_int, C.c_int, C.c_uint, C.POINTER(H)]
    L.npp_destroy.argtypes = [H]
    L.npp_last_error.argtypes = [H]
    L.npp_last_error.restype = C.c_char_p
    L.npp_set_stream.argtypes = [H, C.c_void_p]
    L.npp_sync.argtypes = [H]
    L.npp_load_levels.argtypes = [H, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int]
    L.npp_assign_levels.argtypes = [H, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int]
    L.npp_reset.argtypes = [H, C.POINTER(C.c_uint8)]
    L.npp_reset_ex.argtypes = [H, C.POINTER(C.c_uint8), C.c_int]
    L.npp_set_truncation_limit.argtypes = [H, C.POINTER(C.c_int32), C.c_int32]
    L.npp_step.argtypes = [H, C.c_void_p, C.c_int, C.POINTER(StepOut)]
    L.npp_tick.argtypes = [H, C.c_void_p, C.c_int]
    L.npp_observe.argtypes = [H, C.POINTER(StepOut)]
    L.npp_render_player_frame.argtypes = [H, C.c_void_p]
    L.npp_dump_state.argtypes = [H, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    L.npp_set_ninja_state.argtypes = [H, C.c_int, C.c_int, C.POINTER(C.c_double)]
    L.npp_set_mover_state.argtypes = [H, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    L.npp_dump_movers.argtypes = [H, C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int)]
    L.npp_dump_entities.argtypes = [H, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int)]
    L.npp_dump_level_segments.argtypes = [H, C.c_int, C.POINTER(C.c_int16), C.c_int, C.POINTER(C.c_int)]
    L.npp_compile_level_segments.argtypes = [
        C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_int16), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint32)
    ]
    L.npp_compile_level_entities.argtypes = [C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int)]
    L.npp_set_launch_geometry.argtypes = [H, C.c_int, C.c_int]
    L.npp_set_step_variant.argtypes = [H, C.c_int]
    L.npp_set_obs_overlap.argtypes = [H, C.c_int]
    L.npp_join.argtypes = [H]
    L.npp_set_obs_overlap_parts.argtypes = [H, C.POINTER(C.c_int), C.c_int]
    L.npp_get_step_variant.argtypes = [H, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.npp_get_launch_geometry.argtypes = [H, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.npp_entity_checksum.argtypes = [H, C.c_int, C.c_int, C.POINTER(C.c_double)]
    L.npp_compile_level_zoo.argtypes = [C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int)]
    L.npp_render_global_view.argtypes = [H, C.c_void_p]
    L.npp_switch_states.argtypes = [H, C.c_void_p]
    L.npp_set_entity_pos.argtypes = [H, C.c_int, C.c_int, C.c_double, C.c_double]
    L.npp_step_many.argtypes = [H, C.c_void_p, C.c_int, C.c_int, C.POINTER(StepOut)]
    L.npp_render_frame.argtypes = [H, C.c_int, C.c_int, C.c_void_p]
    L.npp_plan_zoo_block.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.npp_reachability.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p]
    L.npp_reachability_ex.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.npp_reach_compile.argtypes = [C.POINTER(C.c_double), C.c_int64] + [C.c_void_p] * 12
    L.npp_reach_features_host.argtypes = [C.POINTER(C.c_double), C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p]
    L.npp_reach_compile_miss.argtypes = [C.POINTER(C.c_double), C.c_int64] + [C.c_void_p] * 4
    L.npp_reach_rollout_host.argtypes = [C.POINTER(C.c_double), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.npp_set_dynamic_truncation.argtypes = [H, C.c_int]
    L.npp_level_truncation_limit.argtypes = [C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.npp_snapshot.argtypes = [H]
    L.npp_restore.argtypes = [H, C.POINTER(C.c_uint8)]
    L.npp_set_frame_stack.argtypes = [H, C.c_int, C.c_int, C.c_int]
    L.npp_frame_stack_render.argtypes = [H]
    L.npp_frame_stack_push.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.npp_frame_stack_view.argtypes = [H, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.npp_set_level_pool.argtypes = [H, C.POINTER(C.c_double), C.c_int, C.c_uint64]
    L.npp_draw_levels.argtypes = [H, C.POINTER(C.c_uint8)]
    L.npp_get_env_levels.argtypes = [H, C.POINTER(C.c_int32)]
    L.npp_env_level_view.argtypes = [H, C.POINTER(C.c_void_p)]
    L.npp_graph_observation.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.npp_graph_compile.argtypes = [C.POINTER(C.c_double), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.npp_level_pool_draw_host.argtypes = [C.POINTER(C.c_double), C.c_int, C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.c_int,
                                           C.POINTER(C.c_int32)]
    L.npp_set_minimal_observation.argtypes = [H, C.c_int]
    L.npp_minimal_observation.argtypes = [H, C.c_void_p, C.c_void_p]
    L.npp_minimal_encode_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.npp_state_decode_host.argtypes = [C.c_void_p, C.c_void_p]
    L.npp_set_frame_augmentation.argtypes = [H, C.c_int, C.c_double, C.c_double, C.c_uint64]
    L.npp_frame_augment.argtypes = [H, C.c_void_p]
    L.npp_frame_augment_view.argtypes = [H, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    L.npp_frame_augment_params_host.argtypes = [C.c_uint64, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.npp_frame_augment_apply_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.npp_archive_create.argtypes = [H, C.c_int]
    L.npp_archive_store.argtypes = [H, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.npp_archive_restore.argtypes = [H, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.npp_archive_meta_view.argtypes = [H, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.npp_archive_num_slots.argtypes = [H]
    L.npp_archive_record_bytes.argtypes = [H]
    L.npp_archive_cells_create.argtypes = [H, C.c_int, C.c_uint64]
    L.npp_archive_explore.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p]
    L.npp_archive_select.argtypes = [H, C.c_void_p, C.c_void_p]
    L.npp_archive_cells_view.argtypes = [H] + [C.POINTER(C.c_void_p)] * 6
    L.npp_archive_cell_keys_host.argtypes = [C.POINTER(C.c_double), C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                             C.c_void_p]
    L.npp_archive_cell_pick_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p]
    L.npp_set_routes.argtypes = [H, C.c_int]
    L.npp_route_view.argtypes = [H, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
    L.npp_archive_route_view.argtypes = [H, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.npp_route_apply_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    L.npp_set_action_masking.argtypes = [H, C.c_int]
    L.npp_path_action_mask.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p]
    L.npp_path_mask_stats_view.argtypes = [H] + [C.POINTER(C.c_void_p)] * 4
    L.npp_path_direction_host.argtypes = [C.POINTER(C.c_double), C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p]
    L.npp_num_envs.argtypes = [H]
    L.npp_set_reward_mode.argtypes = [H, C.c_int, C.c_void_p]
    L.npp_set_reward_params.argtypes = [H, C.c_void_p]
    L.npp_step_reward.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p]
    L.npp_reward_default_params.argtypes = [C.c_void_p]
    L.npp_reward_level_constants_host.argtypes = [C.POINTER(C.c_double), C.c_int64, C.c_void_p, C.c_void_p]
    L.npp_reward_host.argtypes = [C.POINTER(C.c_double), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.npp_set_reward_waypoints.argtypes = [H, C.c_int, C.c_void_p]
    L.npp_set_waypoint_params.argtypes = [H, C.c_void_p]
    L.npp_step_reward_wp.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.npp_reward_waypoints.argtypes = [H, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int32)]
    L.npp_waypoint_default_params.argtypes = [C.c_void_p]
    L.npp_reward_waypoints_host.argtypes = [C.POINTER(C.c_double), C.c_int64, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.POINTER(C.c_int32), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.npp_waypoint_bonus_host.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_double)]
    L.npp_reward_host_wp.argtypes = [C.POINTER(C.c_double), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                     C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.npp_num_levels.argtypes = [H]
    L.npp_demo_plan_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]
    L.npp_demo_create.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_uint]
    L.npp_demo_destroy.argtypes = [H]
    L.npp_demo_rows.argtypes = [H, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.npp_demo_play.argtypes = [H, C.POINTER(DemoOut)]
    L.npp_archive_seed.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.npp_archive_seed_rows_host.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.npp_set_episode_stats.argtypes = [H, C.c_int]
    L.npp_episode_accumulate.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.npp_episode_restart.argtypes = [H, C.c_void_p, C.c_int]
    L.npp_episode_view.argtypes = [H] + [C.POINTER(C.c_void_p)] * 3
    L.npp_episode_table_reset.argtypes = [H]
    L.npp_episode_apply_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.npp_goal_default_params.argtypes = [C.c_void_p]
    L.npp_set_goal_curriculum.argtypes = [H, C.c_int, C.c_void_p]
    L.npp_goal_set_stage.argtypes = [H, C.c_int, C.c_int]
    L.npp_goal_view.argtypes = [H] + [C.POINTER(C.c_void_p)] * 3 + [C.POINTER(C.c_int)] * 3
    L.npp_goal_tables.argtypes = [H, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    L.npp_goal_stage_positions.argtypes = [H, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.npp_goal_stages_host.argtypes = [C.POINTER(C.c_double), C.c_int64, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                       C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.npp_goal_apply_host.argtypes = [C.c_void_p] * 5 + [C.c_int] * 6 + [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.npp_compile_level_segments_goal.argtypes = [C.POINTER(C.c_double), C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p]
    L.npp_compile_level_entities_goal.argtypes = [C.POINTER(C.c_double), C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p]
    L.npp_reward_level_constants_goal_host.argtypes = [C.POINTER(C.c_double), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.npp_reward_goal_host.argtypes = [C.POINTER(C.c_double), C.c_int64] + [C.c_void_p] * 7 + [C.c_int, C.c_int] + [C.c_void_p] * 6
    L.npp_reach_rollout_goal_host.argtypes = [C.POINTER(C.c_double), C.c_int64] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 3
    L.npp_path_direction_goal_host.argtypes = [C.POINTER(C.c_double), C.c_int64] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 3
    L.npp_sweep_start.argtypes = [H, C.c_void_p, C.c_int]
    L.npp_sweep_stop.argtypes = [H]
    L.npp_sweep_view.argtypes = [H] + [C.POINTER(C.c_void_p)] * 4 + [C.POINTER(C.c_int)]
    L.npp_sweep_assign_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p]
    for name in EXPORTS:
        if name != "npp_last_error":
            getattr(L, name).restype = C.c_int
    _lib = L
    return L


class NppError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("npp error %d: %s" % (code, msg))
        self.code = code


def check(handle, code):
    if code != NPP_OK:
        msg = lib().npp_last_error(handle)
        raise NppError(code, msg.decode() if msg else "?")
