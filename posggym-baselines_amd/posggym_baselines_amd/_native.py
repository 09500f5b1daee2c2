"""ctypes binding of libpomcp_hip.so (include/pomcp.h).

The structs below mirror the C declarations field for field.  The library is
built in-tree by ``posggym_baselines_amd.build`` (hipcc, gfx950) and loaded
from ``posggym_baselines_amd/_lib/``; there is no fallback: if the shared
object is missing, importing the planner raises.
"""
import ctypes as C
import os

LIB_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib")
LIB_PATH = os.environ.get("POMCP_LIB_PATH") or os.path.join(LIB_DIR, "libpomcp_hip.so")

POMCP_ABI_VERSION = 7
POMCP_MAX_TYPE_POLICIES = 8
POMCP_MAX_ACTIONS = 8
POMCP_XREC_STATS = 6


def xrec(num_actions: int) -> int:
    """Doubles per tree in the exchange record (include/pomcp.h POMCP_XREC)."""
    return 2 * num_actions + POMCP_XREC_STATS

POMCP_OK = 0
POMCP_E_INVALID = -1
POMCP_E_HIP = -2
POMCP_E_ARENA = -3
POMCP_E_STATE = -4
POMCP_E_UNSUPPORTED = -5
POMCP_E_NOT_FOUND = -6
POMCP_E_NO_DEVICE = -7

SEL_PUCB, SEL_UCB, SEL_UNIFORM = 0, 1, 2
SEARCH_AUTO, SEARCH_LANE, SEARCH_WAVE = 0, 1, 2   # pomcp_search_kernel
ENV_DRIVING = 1
ENV_PURSUIT_EVASION = 2
ENV_COOPERATIVE_REACHING = 3   # created through pomcp_create_env with a PomcpCrGrid
ENV_PREDATOR_PREY = 4          # created through pomcp_create_env with a PomcpPpGrid

STATUS_NAMES = {
    POMCP_E_INVALID: "POMCP_E_INVALID",
    POMCP_E_HIP: "POMCP_E_HIP",
    POMCP_E_ARENA: "POMCP_E_ARENA",
    POMCP_E_STATE: "POMCP_E_STATE",
    POMCP_E_UNSUPPORTED: "POMCP_E_UNSUPPORTED",
    POMCP_E_NOT_FOUND: "POMCP_E_NOT_FOUND",
    POMCP_E_NO_DEVICE: "POMCP_E_NO_DEVICE",
}


class PomcpGrid(C.Structure):
    _fields_ = [
        ("wall", C.c_uint8 * 256),
        ("dist", (C.c_uint8 * 256) * 8),
        ("loc_x", C.c_uint8 * 8),
        ("loc_y", C.c_uint8 * 8),
        ("loc_dir", C.c_uint8 * 8),
        ("width", C.c_int32),
        ("height", C.c_int32),
        ("num_locs", C.c_int32),
        ("obs_front", C.c_int32),
        ("obs_back", C.c_int32),
        ("obs_side", C.c_int32),
        ("pad", C.c_int32 * 2),
    ]


class PomcpPeGrid(C.Structure):
    _fields_ = [
        ("wall", C.c_uint8 * 256),
        ("goal_dist", (C.c_uint8 * 256) * 4),
        ("evader_start", (C.c_uint8 * 2) * 4),
        ("pursuer_start", (C.c_uint8 * 2) * 4),
        ("goal", (C.c_uint8 * 2) * 4),
        ("width", C.c_int32),
        ("height", C.c_int32),
        ("n_evader_start", C.c_int32),
        ("n_pursuer_start", C.c_int32),
        ("n_goal", C.c_int32),
        ("max_obs_distance", C.c_int32),
        ("use_progress_reward", C.c_int32),
        ("pad", C.c_int32),
        ("reward_norm", C.c_double),
    ]


class PomcpCrGrid(C.Structure):
    _fields_ = [
        ("size", C.c_int32),
        ("obs_distance", C.c_int32),
        ("num_goals", C.c_int32),
        ("pad", C.c_int32),
        ("goal", (C.c_uint8 * 2) * 4),
        ("goal_value", C.c_double * 4),
    ]


class PomcpPpGrid(C.Structure):
    _fields_ = [
        ("size", C.c_int32),
        ("num_prey", C.c_int32),
        ("prey_strength", C.c_int32),
        ("obs_dim", C.c_int32),
        ("start", (C.c_uint8 * 2) * 8),
        ("capture_reward", C.c_double),
    ]


class PomcpConfig(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("env_id", C.c_int32),
        ("num_agents", C.c_int32),
        ("ego_agent", C.c_int32),
        ("num_actions", C.c_int32),
        ("action_selection", C.c_int32),
        ("depth_limit", C.c_int32),
        ("step_limit", C.c_int32),
        ("num_particles", C.c_int32),
        ("extra_particles", C.c_int32),
        ("has_known_bounds", C.c_int32),
        ("num_trees", C.c_int32),
        ("discount", C.c_double),
        ("c", C.c_double),
        ("pucb_exploration_fraction", C.c_double),
        ("reinvigoration_sample_limit_factor", C.c_double),
        ("known_min", C.c_double),
        ("known_max", C.c_double),
        ("seed", C.c_uint64),
        ("tree_key_base", C.c_uint32),
        ("type_based", C.c_int32),
        ("max_blocks", C.c_int64),
        ("max_particles", C.c_int64),
        ("max_belief", C.c_int64),
        ("overflow_slots", C.c_int64),
        ("log_table", C.POINTER(C.c_double)),
        ("log_table_size", C.c_int64),
        ("discount_pow", C.POINTER(C.c_double)),
        ("discount_pow_size", C.c_int64),
        ("grid", PomcpGrid),
        ("pe_grid", PomcpPeGrid),
    ]


class PomcpRootStats(C.Structure):
    _fields_ = [
        ("action", C.c_int32),
        ("num_sims", C.c_int32),
        ("search_depth", C.c_int32),
        ("root_visits", C.c_int32),
        ("root_absorbing", C.c_int32),
        ("belief_size", C.c_int32),
        ("error", C.c_int32),
        ("num_children", C.c_int32),
        ("child_visits", C.c_int32 * POMCP_MAX_ACTIONS),
        ("child_values", C.c_double * POMCP_MAX_ACTIONS),
        ("child_totals", C.c_double * POMCP_MAX_ACTIONS),
        ("min_value", C.c_double),
        ("max_value", C.c_double),
        ("n_levels", C.c_int64),
        ("n_expansions", C.c_int64),
        ("n_new_nodes", C.c_int64),
        ("n_rollout_steps", C.c_int64),
        ("n_probes", C.c_int64),
        ("n_obs_nodes", C.c_int32),
        ("n_blocks", C.c_int32),
        ("n_log", C.c_int32),
        ("n_deferred", C.c_int32),
        ("n_cutoff", C.c_int32),
        ("n_exact_selects", C.c_int32),
    ]


class PomcpMergedRoot(C.Structure):
    """``pomcp_merged_root`` (include/pomcp.h)."""
    _fields_ = [
        ("action", C.c_int32),
        ("num_trees", C.c_int32),
        ("search_depth", C.c_int32),
        ("error", C.c_int32),
        ("num_sims", C.c_int64),
        ("root_visits", C.c_int64),
        ("min_value", C.c_double),
        ("max_value", C.c_double),
        ("visits", C.c_double * POMCP_MAX_ACTIONS),
        ("totals", C.c_double * POMCP_MAX_ACTIONS),
    ]


class PomcpBeliefCounts(C.Structure):
    """``pomcp_belief_counts`` (include/pomcp.h)."""
    _fields_ = [
        ("belief_size", C.c_int32),
        ("state_matches", C.c_int32),
        ("error", C.c_int32),
        ("pad", C.c_int32),
        ("policy_hist", C.c_int32 * POMCP_MAX_TYPE_POLICIES),
    ]


# the same record as a numpy dtype (PomcpEngine.belief_counts)
BELIEF_COUNTS_DTYPE = [("belief_size", "<i4"), ("state_matches", "<i4"), ("error", "<i4"),
                       ("pad", "<i4"), ("policy_hist", "<i4", (POMCP_MAX_TYPE_POLICIES,))]


UNTIL_AGENT_DONE, UNTIL_ALL_DONE = 0, 1   # pomcp_episode_until


class PomcpEpisodeResult(C.Structure):
    """``pomcp_episode_result`` (include/pomcp.h)."""
    _fields_ = [
        ("env_seed", C.c_uint64),
        ("len", C.c_int32),
        ("searched_steps", C.c_int32),
        ("ret", C.c_double),
        ("discounted_return", C.c_double),
        ("ego_terminated", C.c_int32),
        ("all_done", C.c_int32),
        ("truncated", C.c_int32),
        ("error", C.c_int32),
        ("search_depth_sum", C.c_int64),
        ("num_sims_sum", C.c_int64),
        ("min_value_sum", C.c_double),
        ("max_value_sum", C.c_double),
    ]


class PomcpEpisodeState(C.Structure):
    """``pomcp_episode_state`` (include/pomcp.h)."""
    _fields_ = [
        ("res", PomcpEpisodeResult),
        ("v0", C.c_uint32),
        ("v1", C.c_uint32),
        ("model_ctr", C.c_uint32),
        ("policy_ctr", C.c_uint32),
        ("last_action", C.c_int32),
        ("finished", C.c_int32),
        ("root_absorbing", C.c_int32),
        ("last_other_action", C.c_int32),
        ("last_reward", C.c_double),
    ]


class PomcpEpisodeStepIn(C.Structure):
    """``pomcp_episode_step_in`` (include/pomcp.h)."""
    _fields_ = [
        ("root_absorbing", C.c_int32),
        ("action", C.c_int32),
        ("search_depth", C.c_int32),
        ("num_sims", C.c_int32),
        ("error", C.c_int32),
        ("pad", C.c_int32),
        ("min_value", C.c_double),
        ("max_value", C.c_double),
    ]


class PomcpEpisodeStepOut(C.Structure):
    """``pomcp_episode_step_out`` (include/pomcp.h)."""
    _fields_ = [
        ("obs_key", C.c_uint64),
        ("reward", C.c_double),
        ("ego_action", C.c_int32),
        ("other_action", C.c_int32),
        ("stepped", C.c_int32),
        ("pad", C.c_int32),
    ]


class PomcpEpisodePopulation(C.Structure):
    """``pomcp_episode_population`` (include/pomcp.h)."""
    _fields_ = [
        ("num_policies", C.c_int32),
        ("pad", C.c_int32),
        ("pi", (C.c_double * POMCP_MAX_ACTIONS) * POMCP_MAX_TYPE_POLICIES),
        ("mixture_index", C.c_int32 * POMCP_MAX_TYPE_POLICIES),
    ]


class PomcpEpisodePopState(C.Structure):
    """``pomcp_episode_pop_state`` (include/pomcp.h)."""
    _fields_ = [
        ("policy_index", C.c_int32),
        ("mixture_index", C.c_int32),
    ]


POLICY_FIXED, POLICY_DRIVING_SHORTEST_PATH = 0, 1   # pomcp_policy_kinds.kind
POLICY_CR_GOAL = 3                                  # (2 is unassigned)
POLICY_PP_HEURISTIC = 5                             # (4 is unassigned)


class PomcpPolicyKinds(C.Structure):
    """``pomcp_policy_kinds`` (include/pomcp.h)."""
    _fields_ = [
        ("kind", C.c_int32 * POMCP_MAX_TYPE_POLICIES),
        ("param0", C.c_int32 * POMCP_MAX_TYPE_POLICIES),
        ("param1", C.c_int32 * POMCP_MAX_TYPE_POLICIES),
    ]


class PomcpEpisodeBeliefAcc(C.Structure):
    """``pomcp_episode_belief_acc`` (include/pomcp.h)."""
    _fields_ = [
        ("state_sum", C.c_double),
        ("policy_sum", C.c_double),
        ("action_sum", C.c_double),
        ("count", C.c_int32),
        ("error", C.c_int32),
    ]


class PomcpEpisodeQueueRow(C.Structure):
    """``pomcp_episode_queue_row`` (include/pomcp.h)."""
    _fields_ = [
        ("res", PomcpEpisodeResult),
        ("slot", C.c_int32),
        ("slot_order", C.c_int32),
        ("policy_index", C.c_int32),
        ("start_step", C.c_int32),
        ("acc", PomcpEpisodeBeliefAcc),
    ]


EPISODE_POP_STATE_DTYPE = [("policy_index", "<i4"), ("mixture_index", "<i4")]
EPISODE_BELIEF_ACC_DTYPE = [("state_sum", "<f8"), ("policy_sum", "<f8"), ("action_sum", "<f8"),
                            ("count", "<i4"), ("error", "<i4")]

# the same records as numpy dtypes (BatchedPOMCP.run_episodes / episode_states)
EPISODE_RESULT_DTYPE = [("env_seed", "<u8"), ("len", "<i4"), ("searched_steps", "<i4"),
                        ("ret", "<f8"), ("discounted_return", "<f8"), ("ego_terminated", "<i4"),
                        ("all_done", "<i4"), ("truncated", "<i4"), ("error", "<i4"),
                        ("search_depth_sum", "<i8"), ("num_sims_sum", "<i8"),
                        ("min_value_sum", "<f8"), ("max_value_sum", "<f8")]
EPISODE_STATE_DTYPE = [("res", EPISODE_RESULT_DTYPE), ("v0", "<u4"), ("v1", "<u4"),
                       ("model_ctr", "<u4"), ("policy_ctr", "<u4"), ("last_action", "<i4"),
                       ("finished", "<i4"), ("root_absorbing", "<i4"),
                       ("last_other_action", "<i4"), ("last_reward", "<f8")]
EPISODE_QUEUE_ROW_DTYPE = [("res", EPISODE_RESULT_DTYPE), ("slot", "<i4"), ("slot_order", "<i4"),
                           ("policy_index", "<i4"), ("start_step", "<i4"),
                           ("acc", EPISODE_BELIEF_ACC_DTYPE)]


# (name, restype, argtypes) for every symbol include/pomcp.h declares.
_CTX = C.c_void_p
class PomcpTypePolicies(C.Structure):
    """``pomcp_type_policies`` (include/pomcp.h): POTMMCP's fixed-distribution policies."""
    _fields_ = [
        ("num_ego", C.c_int32),
        ("num_other", C.c_int32),
        ("ego_pi", (C.c_double * POMCP_MAX_ACTIONS) * POMCP_MAX_TYPE_POLICIES),
        ("other_pi", (C.c_double * POMCP_MAX_ACTIONS) * POMCP_MAX_TYPE_POLICIES),
        ("meta_len", C.c_int32 * POMCP_MAX_TYPE_POLICIES),
        ("meta_policy", (C.c_int32 * POMCP_MAX_TYPE_POLICIES) * POMCP_MAX_TYPE_POLICIES),
        ("meta_weight", (C.c_double * POMCP_MAX_TYPE_POLICIES) * POMCP_MAX_TYPE_POLICIES),
        ("expected_prior", C.c_double * POMCP_MAX_ACTIONS),
        ("no_meta_draw", C.c_int32),
        ("no_mixture_draw", C.c_int32),
        ("ego_uniform", C.c_int32),
        ("other_uniform", C.c_int32),
    ]


_P32 = C.POINTER(C.c_int32)
_PU32 = C.POINTER(C.c_uint32)
_PU64 = C.POINTER(C.c_uint64)
_PD = C.POINTER(C.c_double)
SIGNATURES = [
    ("pomcp_abi_version", C.c_int32, []),
    ("pomcp_create", C.c_int, [C.POINTER(PomcpConfig), C.c_int32, C.c_void_p, C.POINTER(_CTX)]),
    ("pomcp_create_env", C.c_int,
     [C.POINTER(PomcpConfig), C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.POINTER(_CTX)]),
    ("pomcp_destroy", None, [_CTX]),
    ("pomcp_last_error", C.c_char_p, [_CTX]),
    ("pomcp_set_stream", C.c_int, [_CTX, C.c_void_p]),
    ("pomcp_reset", C.c_int, [_CTX]),
    ("pomcp_update", C.c_int, [_CTX, _P32, _PU64, _P32]),
    ("pomcp_search", C.c_int, [_CTX, C.c_int32, _P32]),
    ("pomcp_search_continue", C.c_int, [_CTX, C.c_int32]),
    ("pomcp_set_search_kernel", C.c_int, [_CTX, C.c_int32]),
    ("pomcp_search_kernel_used", C.c_int32, [_CTX]),
    ("pomcp_set_defer_cutoff", C.c_int, [_CTX, C.c_int32]),
    ("pomcp_get_root_stats", C.c_int, [_CTX, C.POINTER(PomcpRootStats)]),
    ("pomcp_set_root_belief", C.c_int, [_CTX, C.c_int32, _PU32, C.c_int32]),
    ("pomcp_get_root_belief", C.c_int, [_CTX, C.c_int32, _PU32, C.c_int32, _P32]),
    ("pomcp_set_type_policies", C.c_int, [_CTX, C.POINTER(PomcpTypePolicies)]),
    ("pomcp_get_root_prior", C.c_int, [_CTX, C.c_int32, _PD]),
    ("pomcp_get_root_policies", C.c_int, [_CTX, C.c_int32, _P32, C.c_int32, _P32]),
    ("pomcp_belief_stats", C.c_int, [_CTX, _PU32, C.POINTER(PomcpBeliefCounts)]),
    ("pomcp_arena_usage", C.c_int, [_CTX, _P32, _P32]),
    ("pomcp_rekey", C.c_int, [_CTX, C.c_uint64]),
    ("pomcp_root_merge_buffer", C.c_int, [_CTX, C.POINTER(C.c_void_p)]),
    ("pomcp_root_gather_buffer", C.c_int, [_CTX, C.c_int32, C.POINTER(C.c_void_p)]),
    ("pomcp_allgather_root", C.c_int, [_CTX, C.c_void_p, C.c_int32]),
    ("pomcp_merge_roots", C.c_int, [_CTX, C.c_int32, C.c_int32, C.POINTER(PomcpMergedRoot)]),
    ("pomcp_synthetic_obs", C.c_int, [_CTX, C.c_uint64, _PU64]),
    ("pomcp_synthetic_step", C.c_int, [_CTX, C.c_uint64, _P32, _PU64]),
    ("pomcp_snapshot", C.c_int, [_CTX]),
    ("pomcp_restore", C.c_int, [_CTX]),
    ("pomcp_driving_sample_initial_state", C.c_int,
     [C.POINTER(PomcpGrid), C.c_uint64, C.c_uint32, _PU32, _PU32]),
    ("pomcp_driving_step", C.c_int,
     [C.POINTER(PomcpGrid), C.c_uint64, C.c_uint32, _PU32, _PU32, _P32, _PU32, _PD, _P32, _PU64]),
    ("pomcp_driving_obs", C.c_int, [C.POINTER(PomcpGrid), _PU32, _PU64]),
    ("pomcp_pe_sample_initial_state", C.c_int,
     [C.POINTER(PomcpPeGrid), C.c_uint64, C.c_uint32, _PU32, _PU32]),
    ("pomcp_pe_step", C.c_int, [C.POINTER(PomcpPeGrid), _PU32, _P32, _PU32, _PD, _P32, _PU64]),
    ("pomcp_pe_obs", C.c_int, [C.POINTER(PomcpPeGrid), _PU32, _PU64]),
    ("pomcp_cr_sample_initial_state", C.c_int,
     [C.POINTER(PomcpCrGrid), C.c_uint64, C.c_uint32, _PU32, _PU32]),
    ("pomcp_cr_step", C.c_int, [C.POINTER(PomcpCrGrid), _PU32, _P32, _PU32, _PD, _P32, _PU64]),
    ("pomcp_cr_obs", C.c_int, [C.POINTER(PomcpCrGrid), _PU32, _PU64]),
    ("pomcp_cr_sample_agent_initial_state", C.c_int,
     [C.POINTER(PomcpCrGrid), C.c_int32, C.c_uint64, C.c_uint64, C.c_uint32, _PU32, _PU32]),
    ("pomcp_pp_sample_initial_state", C.c_int,
     [C.POINTER(PomcpPpGrid), C.c_uint64, C.c_uint32, _PU32, _PU32]),
    ("pomcp_pp_step", C.c_int, [C.POINTER(PomcpPpGrid), _PU32, _P32, C.c_uint64, C.c_uint32, _PU32,
                                _PU32, _PD, _P32, _PU64]),
    ("pomcp_debug_pp_step_draw", C.c_int, [C.POINTER(PomcpPpGrid), _PU32, _P32, C.c_uint32, _PU32,
                                           _PD, _P32, _PU64, _P32, _P32]),
    ("pomcp_pp_obs", C.c_int, [C.POINTER(PomcpPpGrid), _PU32, _PU64]),
    ("pomcp_pp_sample_agent_initial_state", C.c_int,
     [C.POINTER(PomcpPpGrid), C.c_int32, C.c_uint64, C.c_uint64, C.c_uint32, _PU32, _PU32]),
    ("pomcp_host_cr_policy_actions", C.c_int,
     [C.POINTER(PomcpCrGrid), C.c_int64, _PU32, C.c_int32, _P32]),
    ("pomcp_host_pp_policy_pi", C.c_int,
     [C.POINTER(PomcpPpGrid), C.c_int64, _PU32, _PU32, C.c_int32, C.c_int32, _PD]),
    ("pomcp_host_pp_policy_actions", C.c_int,
     [C.POINTER(PomcpPpGrid), C.c_int64, _PU32, _PU32, C.c_int32, C.c_int32, _PU32, _P32]),
    ("pomcp_philox_words", C.c_int, [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32,
                                     _PU32]),
    ("pomcp_host_log_table", C.c_int, [C.c_int64, C.c_int64, _PD]),
    ("pomcp_host_belief_counts", C.c_int,
     [_PU32, C.c_int64, _PU32, C.c_int32, C.POINTER(PomcpBeliefCounts)]),
    ("pomcp_episodes_begin", C.c_int, [_CTX, _PU64, _PD, C.c_int32, C.c_int32]),
    ("pomcp_episodes_step", C.c_int, [_CTX, C.c_int32, _P32]),
    ("pomcp_episodes_results", C.c_int, [_CTX, C.POINTER(PomcpEpisodeResult)]),
    ("pomcp_episodes_states", C.c_int, [_CTX, C.POINTER(PomcpEpisodeState)]),
    ("pomcp_episodes_track_states", C.c_int, [_CTX, C.c_int32]),
    ("pomcp_episodes_belief_stats", C.c_int, [_CTX, C.POINTER(PomcpBeliefCounts)]),
    ("pomcp_episodes_timing", C.c_int, [_CTX, _PD, _P32]),
    ("pomcp_host_episode_reset", C.c_int,
     [C.c_int32, C.c_void_p, C.c_int32, C.c_uint64, C.POINTER(PomcpEpisodeState), _PU64]),
    ("pomcp_host_episode_step", C.c_int,
     [C.c_int32, C.c_void_p, C.c_int32, C.POINTER(PomcpEpisodeStepIn), _PD, C.c_int32, C.c_int32,
      C.POINTER(PomcpEpisodeState), C.POINTER(PomcpEpisodeStepOut)]),
    ("pomcp_episodes_set_population", C.c_int, [_CTX, C.POINTER(PomcpEpisodePopulation)]),
    ("pomcp_episodes_pop_states", C.c_int, [_CTX, C.POINTER(PomcpEpisodePopState)]),
    ("pomcp_episodes_track_belief_acc", C.c_int, [_CTX, C.c_int32, C.c_int32]),
    ("pomcp_episodes_belief_acc", C.c_int, [_CTX, C.POINTER(PomcpEpisodeBeliefAcc)]),
    ("pomcp_episodes_belief_acc_steps", C.c_int, [_CTX, _PD]),
    ("pomcp_episodes_belief_acc_ms", C.c_int, [_CTX, _PD]),
    ("pomcp_host_episode_reset_pop", C.c_int,
     [C.c_int32, C.c_void_p, C.c_int32, C.c_uint64, C.POINTER(PomcpEpisodePopulation),
      C.POINTER(PomcpEpisodeState), C.POINTER(PomcpEpisodePopState), _PU64]),
    ("pomcp_host_episode_step_pop", C.c_int,
     [C.c_int32, C.c_void_p, C.c_int32, C.POINTER(PomcpEpisodeStepIn), _PD, C.c_int32, C.c_int32,
      C.POINTER(PomcpEpisodePopulation), C.POINTER(PomcpEpisodePopState),
      C.POINTER(PomcpEpisodeState), C.POINTER(PomcpEpisodeStepOut)]),
    ("pomcp_host_belief_acc", C.c_int,
     [C.POINTER(PomcpBeliefCounts), C.c_int32, C.c_int32, _PD, C.c_int32, _PD]),
    ("pomcp_episodes_set_population_kinds", C.c_int, [_CTX, C.POINTER(PomcpPolicyKinds)]),
    ("pomcp_set_type_policy_kinds", C.c_int, [_CTX, C.POINTER(PomcpPolicyKinds)]),
    ("pomcp_set_type_ego_kinds", C.c_int, [_CTX, C.POINTER(PomcpPolicyKinds), _PD]),
    ("pomcp_host_cr_prior_lines", C.c_int,
     [C.POINTER(PomcpCrGrid), C.c_int32, _PD, _PD, C.POINTER(PomcpPolicyKinds), _PD, C.c_int32,
      C.c_int64, _PU32, _PD]),
    ("pomcp_host_driving_policy_actions", C.c_int,
     [C.POINTER(PomcpGrid), C.c_int64, _PU32, _PU32, C.c_int32, C.c_int32, _P32]),
    ("pomcp_host_episode_step_pop_kinds", C.c_int,
     [C.c_int32, C.c_void_p, C.c_int32, C.POINTER(PomcpEpisodeStepIn), _PD, C.c_int32, C.c_int32,
      C.POINTER(PomcpEpisodePopulation), C.POINTER(PomcpPolicyKinds),
      C.POINTER(PomcpEpisodePopState), C.POINTER(PomcpEpisodeState),
      C.POINTER(PomcpEpisodeStepOut)]),
    ("pomcp_episodes_queue_begin", C.c_int, [_CTX, _PU64, C.c_int32, _PD, C.c_int32, C.c_int32]),
    ("pomcp_episodes_queue_rows", C.c_int, [_CTX, C.POINTER(PomcpEpisodeQueueRow)]),
    ("pomcp_episodes_queue_slots", C.c_int, [_CTX, _P32]),
    ("pomcp_episodes_queue_finished", C.c_int, [_CTX, C.POINTER(PomcpEpisodeState), _P32]),
    ("pomcp_episodes_queue_timing", C.c_int, [_CTX, _PD]),
    ("pomcp_host_log_drop", C.c_int,
     [_PU32, _PU32, _PU32, _PU32, C.c_int64, C.c_uint64, C.POINTER(C.c_int64)]),
    ("pomcp_host_queue_assign", C.c_int, [_P32, _P32, C.c_int32, C.c_int32, _P32, _P32, _P32]),
    ("pomcp_episodes_set_group", C.c_int, [_CTX, C.c_int32]),
    ("pomcp_episodes_merged_roots", C.c_int, [_CTX, C.POINTER(PomcpMergedRoot)]),
    ("pomcp_host_episode_group_step_in", C.c_int,
     [_P32, C.c_int32, C.c_int32, C.POINTER(PomcpMergedRoot), C.POINTER(PomcpEpisodeStepIn), _P32]),
    ("pomcp_episodes_group_queue_begin", C.c_int,
     [_CTX, C.c_int32, _PU64, C.c_int32, _PD, C.c_int32, C.c_int32]),
    ("pomcp_episodes_queue_finished_merged", C.c_int, [_CTX, C.POINTER(PomcpMergedRoot)]),
    ("pomcp_host_group_drop_masks", C.c_int, [_P32, C.c_int32, C.c_int32, C.c_int32, _PU64]),
]
DEBUG_SIGNATURES = [
    ("pomcp_debug_fp_selftest", C.c_int, [_PD, _PD, C.c_int32, _PD]),
    ("pomcp_debug_exp", C.c_int, [_PD, C.c_int32, _PD]),
    ("pomcp_debug_fast_recip", C.c_int, [_PD, C.c_int32, _PD]),
    ("pomcp_debug_host_exp", C.c_int, [_PD, C.c_int32, _PD]),
    ("pomcp_debug_phase_timing", C.c_int,
     [C.c_void_p, C.POINTER(C.c_uint64), C.c_int32, C.POINTER(C.c_int32)]),
    ("pomcp_debug_set_inline_slots", C.c_int, [C.c_void_p, C.c_int32]),
    ("pomcp_debug_set_map_generation", C.c_int, [C.c_void_p, _P32]),
    ("pomcp_debug_map_scan", C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]),
    ("pomcp_debug_set_select_margin", C.c_int, [C.c_void_p, C.c_double]),
    ("pomcp_debug_set_spin_limit", C.c_int, [C.c_void_p, C.c_int32]),
    ("pomcp_debug_belief_stats_ms", C.c_int,
     [C.c_void_p, _PU32, C.c_int32, C.POINTER(C.c_float)]),
    ("pomcp_debug_search_depth_spec", C.c_int, [C.c_void_p]),
    ("pomcp_debug_get_wave_log", C.c_int,
     [C.c_void_p, C.c_int32, _PU32, _PU32, _PU32, _PU32, C.c_int32, _P32]),
    ("pomcp_debug_log_drop", C.c_int, [C.c_void_p, _PU64]),
    ("pomcp_debug_env_step", C.c_int, [C.c_void_p, _PU32, C.c_int32, _PU32]),
    ("intmcp_debug_set_softmax_slack", C.c_int, [C.c_void_p, C.c_float]),
    ("intmcp_debug_exact_draws", C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    ("intmcp_debug_arena_scan", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    ("intmcp_debug_queue_cleared_bytes", C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
]



class IntmcpConfig(C.Structure):
    """``intmcp_config`` (include/intmcp.h)."""
    _fields_ = [
        ("base", PomcpConfig),
        ("state_belief_only", C.c_int32),
        ("nesting_level", C.c_int32),
        ("max_nodes", C.c_int64),
        ("max_stats", C.c_int64),
        ("max_log", C.c_int64),
        ("hash_slots", C.c_int64),
        ("max_root_belief", C.c_int64),
        ("max_support_particles", C.c_int64),
    ]


class IntmcpRootStats(C.Structure):
    """``intmcp_root_stats`` (include/intmcp.h)."""
    _fields_ = [
        ("action", C.c_int32),
        ("num_sims", C.c_int32),
        ("search_depth", C.c_int32),
        ("root_visits", C.c_int32),
        ("root_absorbing", C.c_int32),
        ("belief_size", C.c_int32),
        ("error", C.c_int32),
        ("num_children", C.c_int32),
        ("child_action", C.c_int32 * POMCP_MAX_ACTIONS),
        ("child_visits", C.c_int32 * POMCP_MAX_ACTIONS),
        ("child_values", C.c_double * POMCP_MAX_ACTIONS),
        ("child_totals", C.c_double * POMCP_MAX_ACTIONS),
        ("min_value", C.c_double),
        ("max_value", C.c_double),
        ("n_nodes", C.c_int32 * 2),
        ("n_log", C.c_int32 * 2),
        ("n_stats", C.c_int32 * 2),
        ("n_support", C.c_int32),
        ("pad", C.c_int32),
    ]


class IntmcpEpisodeRoot(C.Structure):
    """``intmcp_episode_root`` (include/intmcp.h)."""
    _fields_ = [
        ("last_action", C.c_int32),
        ("num_sims", C.c_int32),
        ("search_depth", C.c_int32),
        ("err", C.c_int32),
        ("min_value", C.c_double),
        ("max_value", C.c_double),
        ("info", C.c_uint32),
        ("pad", C.c_int32),
    ]


class IntmcpEpisodeKept(C.Structure):
    """``intmcp_episode_kept`` (include/intmcp.h)."""
    _fields_ = [
        ("info", C.c_uint32),
        ("last_action", C.c_int32),
        ("num_sims", C.c_int32),
        ("search_depth", C.c_int32),
        ("parked", C.c_int32),
        ("pad", C.c_int32 * 3),
    ]


INTMCP_BEGIN, INTMCP_FINAL = 1, 2
INTMCP_SKIP = -2
INTMCP_EPISODE_KEEP_INPUT = -3   # intmcp_host_episode_step: the pair was finished before
INTMCP_ABSORBING_BIT = 1 << 3    # of a node's info word

# numpy views of the diagnostic records (include/intmcp.h)
INTMCP_NODE_DTYPE = [("parent", "<i4"), ("info", "<u4"), ("visits", "<i4"), ("t", "<i4"),
                     ("stats", "<i4"), ("support", "<u4"), ("okey", "<u8")]
INTMCP_STAT_DTYPE = [("visits", "<i4"), ("pad", "<i4"), ("value", "<f8"), ("total", "<f8"),
                     ("agg", "<f8")]
INTMCP_SUPPORT_DTYPE = [("node", "<i4"), ("off", "<i4"), ("size", "<i4"), ("cap", "<i4")]

INTMCP_SIGNATURES = [
    ("intmcp_create", C.c_int, [C.POINTER(IntmcpConfig), C.c_int32, C.c_void_p, C.POINTER(_CTX)]),
    ("intmcp_destroy", None, [_CTX]),
    ("intmcp_last_error", C.c_char_p, [_CTX]),
    ("intmcp_reset", C.c_int, [_CTX]),
    ("intmcp_update", C.c_int, [_CTX, _P32, _PU64, _P32]),
    ("intmcp_search", C.c_int, [_CTX, C.c_int32, _P32]),
    ("intmcp_search_levels", C.c_int, [_CTX, C.c_int32, C.c_int32, C.c_int32, _P32]),
    ("intmcp_get_root_stats", C.c_int, [_CTX, C.POINTER(IntmcpRootStats)]),
    ("intmcp_get_root_belief", C.c_int, [_CTX, C.c_int32, _PU32, C.c_int32, _P32]),
    ("intmcp_get_nodes", C.c_int, [_CTX, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, _P32]),
    ("intmcp_get_stats", C.c_int, [_CTX, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, _P32]),
    ("intmcp_get_support", C.c_int,
     [_CTX, C.c_int32, _P32, C.c_int32, _P32, _PU32, C.c_int32, _P32]),
    ("intmcp_get_mid_support", C.c_int,
     [_CTX, C.c_int32, _P32, C.c_int32, _P32, _PU32, C.c_int32, _P32]),
    ("intmcp_get_middle_support", C.c_int,
     [_CTX, C.c_int32, C.c_int32, _P32, C.c_int32, _P32, _PU32, C.c_int32, _P32]),
    ("intmcp_search_level", C.c_int, [_CTX, C.c_int32, C.c_int32, C.c_int32, _P32]),
    ("intmcp_get_tree_counts", C.c_int, [_CTX, _P32]),
    ("intmcp_synthetic_obs", C.c_int, [_CTX, C.c_uint64, _PU64]),
    ("intmcp_set_search_policy", C.c_int, [_CTX, C.c_int32, C.c_int32, _PD]),
    ("intmcp_debug_phase_timing", C.c_int, [_CTX, C.c_void_p, C.c_int32, _P32]),
    ("intmcp_episodes_set_population", C.c_int, [_CTX, C.POINTER(PomcpEpisodePopulation)]),
    ("intmcp_episodes_begin", C.c_int, [_CTX, _PU64, _PD, C.c_int32, C.c_int32]),
    ("intmcp_episodes_step", C.c_int, [_CTX, C.c_int32, _P32]),
    ("intmcp_episodes_results", C.c_int, [_CTX, C.POINTER(PomcpEpisodeResult)]),
    ("intmcp_episodes_states", C.c_int, [_CTX, C.POINTER(PomcpEpisodeState)]),
    ("intmcp_episodes_pop_states", C.c_int, [_CTX, C.POINTER(PomcpEpisodePopState)]),
    ("intmcp_episodes_timing", C.c_int, [_CTX, _PD, _P32]),
    ("intmcp_host_episode_step", C.c_int,
     [C.c_int32, C.c_void_p, C.c_int32, C.POINTER(IntmcpEpisodeRoot), C.POINTER(IntmcpEpisodeKept),
      _PD, C.c_int32, C.c_int32, C.POINTER(PomcpEpisodePopulation),
      C.POINTER(PomcpEpisodePopState), C.POINTER(PomcpEpisodeState),
      C.POINTER(PomcpEpisodeStepOut), _P32]),
    ("intmcp_host_episode_unpark", C.c_int,
     [C.POINTER(IntmcpEpisodeRoot), C.POINTER(IntmcpEpisodeKept), _P32]),
    ("intmcp_reset_pairs", C.c_int, [_CTX, _P32, C.c_int32]),
    ("intmcp_episodes_queue_begin", C.c_int, [_CTX, _PU64, C.c_int32, _PD, C.c_int32, C.c_int32]),
    ("intmcp_episodes_queue_rows", C.c_int, [_CTX, C.POINTER(PomcpEpisodeQueueRow)]),
    ("intmcp_episodes_queue_slots", C.c_int, [_CTX, _P32]),
    ("intmcp_episodes_queue_finished", C.c_int, [_CTX, C.POINTER(PomcpEpisodeState), _P32]),
    ("intmcp_episodes_queue_timing", C.c_int, [_CTX, _PD]),
    ("intmcp_host_episode_refill", C.c_int, [C.c_int32, C.POINTER(IntmcpEpisodeKept), _P32, _P32]),
]

_lib = None


class PomcpError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{STATUS_NAMES.get(code, code)}: {msg}")
        self.code = code


def load():
    """Load the in-tree shared object (raises if it was never built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -m posggym_baselines_amd.build` "
            "(or __graft_entry__.build()); there is no CPU fallback for the planner")
    # One HIP runtime per process: PyTorch ships its own libamdhip64.so.7 (same
    # soname as /opt/rocm's).  Whichever loads first serves both; torch only
    # initialises on its own copy, so it is loaded before this library.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, res, args in SIGNATURES + DEBUG_SIGNATURES + INTMCP_SIGNATURES:
        if (name, res, args) in DEBUG_SIGNATURES and not hasattr(lib, name):
            continue   # diagnostics: optional in libraries built from older sources
        if os.environ.get("POMCP_LIB_PATH") and not hasattr(lib, name):
            continue   # an explicitly chosen (measurement) library built from older sources
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.pomcp_abi_version() != POMCP_ABI_VERSION:
        raise ImportError("libpomcp_hip.so ABI version mismatch; rebuild")
    _lib = lib
    return lib


def check(rc, ctx=None, what="", last_error="pomcp_last_error"):
    if rc != POMCP_OK:
        msg = what
        if ctx is not None:
            err = getattr(load(), last_error)(ctx)
            if err:
                msg = f"{what}: {err.decode()}"
        raise PomcpError(rc, msg)
