/* pomcp.h — C ABI of the MI355X-native POMCP engine (libpomcp_hip.so).
 *
 * Drop-in boundary for the hot path of posggym_baselines.planning
 * (SURVEY §8(b)).  Plain pointers and sizes only; no torch types.  Every entry
 * point replaces a piece of the reference planner, cited per function below
 * (paths relative to posggym_baselines/planning/ in the reference).
 *
 * Threading: a context is not thread-safe (the reference planner objects are
 * single-threaded).  Host buffers are copied synchronously unless noted.
 * Return codes: POMCP_OK (0) or a negative pomcp_status; pomcp_last_error()
 * gives the message.
 */
#ifndef POMCP_H_
#define POMCP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define POMCP_ABI_VERSION 7
#define POMCP_MAX_ACTIONS 8
#define POMCP_MAX_TYPE_POLICIES 8

typedef enum pomcp_status {
  POMCP_OK = 0,
  POMCP_E_INVALID = -1,      /* bad argument / config (MCTSConfig.__post_init__ asserts) */
  POMCP_E_HIP = -2,          /* HIP runtime error */
  POMCP_E_ARENA = -3,        /* per-tree arena capacity exceeded */
  POMCP_E_STATE = -4,        /* call out of order (e.g. search before update) */
  POMCP_E_UNSUPPORTED = -5,  /* model / option not implemented on the GPU */
  POMCP_E_NOT_FOUND = -6,    /* node.py:58-63 AssertionError: root has no child for action */
  POMCP_E_NO_DEVICE = -7
} pomcp_status;

typedef enum pomcp_selection {
  POMCP_SEL_PUCB = 0,     /* mcts.py:492-527 + max_visit final (565-581) */
  POMCP_SEL_UCB = 1,      /* mcts.py:529-546 + max_value final (583-600) */
  POMCP_SEL_UNIFORM = 2   /* mcts.py:548-563 + max_value final */
} pomcp_selection;

typedef enum pomcp_env {
  POMCP_ENV_DRIVING = 1,            /* Driving-v1: pomcp_config.grid */
  POMCP_ENV_PURSUIT_EVASION = 2,    /* PursuitEvasion-v1: pomcp_config.pe_grid */
  POMCP_ENV_COOPERATIVE_REACHING = 3,  /* CooperativeReaching-v0: a pomcp_cr_grid beside the
                                          config (pomcp_create_env) */
  POMCP_ENV_PREDATOR_PREY = 4          /* PredatorPrey-v0: a pomcp_pp_grid beside the config
                                          (pomcp_create_env) */
} pomcp_env;

/* Driving-v1 grid tables (16-wide row stride). */
typedef struct pomcp_grid {
  uint8_t wall[256];
  uint8_t dist[8][256];
  uint8_t loc_x[8], loc_y[8], loc_dir[8];
  int32_t width, height, num_locs;
  int32_t obs_front, obs_back, obs_side;
  int32_t pad[2];
} pomcp_grid;

/* PursuitEvasion-v1 grid (16-wide row stride; coordinates are (x, y)). */
typedef struct pomcp_pe_grid {
  uint8_t wall[256];
  uint8_t goal_dist[4][256];      /* BFS distance to goal k (127 = unreachable) */
  uint8_t evader_start[4][2], pursuer_start[4][2], goal[4][2];
  int32_t width, height, n_evader_start, n_pursuer_start, n_goal, max_obs_distance;
  int32_t use_progress_reward, pad;
  double reward_norm;             /* R_MAX + R_PROGRESS * longest start-goal path */
} pomcp_pe_grid;

/* CooperativeReaching-v0 (csrc/cooperative_reaching.h): an S x S grid with a
 * goal in every corner; coordinates are (x, y). */
typedef struct pomcp_cr_grid {
  int32_t size;                   /* S, 3..8 */
  int32_t obs_distance;           /* Chebyshev distance the other agent is seen at; -1: always */
  int32_t num_goals;              /* 4 */
  int32_t pad;
  uint8_t goal[4][2];             /* one per corner */
  double goal_value[4];           /* the reward of both agents on goal k */
} pomcp_cr_grid;

/* PredatorPrey-v0 (csrc/predator_prey.h): two predators and num_prey prey on an
 * open S x S grid; coordinates are (x, y). */
typedef struct pomcp_pp_grid {
  int32_t size;                   /* S: 5 or 10 */
  int32_t num_prey;               /* 1..3 */
  int32_t prey_strength;          /* predators beside a prey that catch it: 1..2 */
  int32_t obs_dim;                /* the observation window reaches this far: 1..2 */
  uint8_t start[8][2];            /* the predators' start cells in row-major order: the
                                     corners and the edge cells at x or y = S / 2 */
  double capture_reward;          /* (double)(float)(1.0 / num_prey), per prey caught */
} pomcp_pp_grid;

/* MCTSConfig (config.py:8-55) after __post_init__, plus engine sizing. */
typedef struct pomcp_config {
  int32_t abi_version;          /* = POMCP_ABI_VERSION */
  int32_t env_id;               /* pomcp_env */
  int32_t num_agents;           /* model.possible_agents (2) */
  int32_t ego_agent;            /* index of agent_id in possible_agents */
  int32_t num_actions;          /* model.action_spaces[agent_id].n */
  int32_t action_selection;     /* pomcp_selection */
  int32_t depth_limit;          /* config.py:50-55 */
  int32_t step_limit;           /* mcts.py:53-58; INT32_MAX = unbounded */
  int32_t num_particles;        /* config.py:47 */
  int32_t extra_particles;      /* config.py:48 */
  int32_t has_known_bounds;
  int32_t num_trees;            /* independent planners (batched roots) */
  double discount;
  double c;
  double pucb_exploration_fraction;
  double reinvigoration_sample_limit_factor;
  double known_min, known_max;
  uint64_t seed;                /* MCTSConfig.seed -> stream key (seed, tree) */
  uint32_t tree_key_base;       /* tree t uses key tree_key_base + t */
  int32_t type_based;           /* 1: POTMMCP's type-based search (pomcp_set_type_policies) */
  /* per-tree arena capacities */
  int64_t max_blocks;           /* expanded obs nodes: A x 128 B action nodes each */
  int64_t max_particles;        /* particle log records (16 B) */
  int64_t max_belief;           /* root belief region (16 B records): the root belief and
                                   the one a re-root builds, one from each end (ABI 7;
                                   was one of two ping-pong buffers); < 2^31 */
  int64_t overflow_slots;       /* children beyond 6 per action node; power of two >= 16 */
  /* host-computed FP64 tables (Python's own math.log / float.__pow__) */
  const double* log_table;      /* log_table[n] = math.log(n), n >= 1 */
  int64_t log_table_size;
  const double* discount_pow;   /* discount ** k */
  int64_t discount_pow_size;
  pomcp_grid grid;              /* env_id == POMCP_ENV_DRIVING */
  pomcp_pe_grid pe_grid;        /* env_id == POMCP_ENV_PURSUIT_EVASION */
} pomcp_config;

/* Per-tree result of the last search (MCTS.step_statistics + root children). */
typedef struct pomcp_root_stats {
  int32_t action;               /* _final_action_selection(root) */
  int32_t num_sims;
  int32_t search_depth;
  int32_t root_visits;
  int32_t root_absorbing;
  int32_t belief_size;
  int32_t error;                /* pomcp_status of this tree */
  int32_t num_children;
  int32_t child_visits[POMCP_MAX_ACTIONS];
  double child_values[POMCP_MAX_ACTIONS];
  double child_totals[POMCP_MAX_ACTIONS];
  double min_value, max_value;  /* MinMaxStats (utils.py:15-42) */
  /* work counters (algorithmic-byte accounting) */
  int64_t n_levels;             /* tree levels stepped (mcts.py:330-381) */
  int64_t n_expansions;         /* leaf expansions (mcts.py:318-321) */
  int64_t n_new_nodes;          /* obs nodes created (mcts.py:369); with deferred cut-off
                                   records (pomcp_set_defer_cutoff) the children first
                                   reached by those records are not included -- they are
                                   created at the next re-root, if they survive it */
  int64_t n_rollout_steps;      /* model steps in _rollout (mcts.py:414-450) */
  int64_t n_probes;             /* obs-child hash bucket probes */
  int32_t n_obs_nodes, n_blocks, n_log;
  int32_t n_deferred;           /* levels whose child (beyond the depth / step limits) was
                                   not looked up: deferred records */
  int32_t n_cutoff;             /* levels below the root whose child lies beyond the depth /
                                   step limits (mcts.py:315), deferred or looked up; their
                                   child slot is not rewritten (0: the wave kernel) */
  int32_t n_exact_selects;      /* UCB / PUCB selections decided by the exact FP64 scores
                                   (near-ties of the fast scores, DESIGN.md §4 "Fast
                                   selection"; pomcp_debug_set_select_margin widens it) */
} pomcp_root_stats;

typedef struct pomcp_ctx pomcp_ctx;

/* Library / ABI identity. */
int32_t pomcp_abi_version(void);

/* MCTS.__init__ (mcts.py:29-91): allocate all per-tree device state.
 * `hip_stream` is a hipStream_t (NULL = the library's own stream). */
int pomcp_create(const pomcp_config* cfg, int32_t device, void* hip_stream, pomcp_ctx** out);
/* pomcp_create for an environment whose description travels beside the config
 * (ABI 7, additive; pomcp_config does not grow): POMCP_ENV_COOPERATIVE_REACHING,
 * env_desc its pomcp_cr_grid and env_desc_bytes that struct's sizeof, or
 * POMCP_ENV_PREDATOR_PREY with its pomcp_pp_grid.
 * pomcp_create refuses those env_ids, and this call every other
 * (POMCP_E_UNSUPPORTED).  These environments run the tree-per-lane search only
 * (pomcp_set_search_kernel(POMCP_SEARCH_WAVE): POMCP_E_UNSUPPORTED). */
int pomcp_create_env(const pomcp_config* cfg, const void* env_desc, int64_t env_desc_bytes,
                     int32_t device, void* hip_stream, pomcp_ctx** out);
void pomcp_destroy(pomcp_ctx* ctx);
const char* pomcp_last_error(const pomcp_ctx* ctx);
int pomcp_set_stream(pomcp_ctx* ctx, void* hip_stream);

/* MCTS.reset (mcts.py:123-138) for every tree: fresh root, t=0; RNG
 * counters persist (the reference's generators are not reseeded). */
int pomcp_reset(pomcp_ctx* ctx);

/* MCTS.update (mcts.py:159-263) for every tree: at t == 0 the initial
 * belief (_initial_update, mcts.py:175-227), else re-root to child
 * (action, obs) and reinvigorate (mcts.py:651-700, belief.py:145-194).
 * obs_keys: packed ego observations (driving.h).  root_absorbing_out may be NULL. */
int pomcp_update(pomcp_ctx* ctx, const int32_t* actions, const uint64_t* obs_keys,
                 int32_t* root_absorbing_out);

/* MCTS.get_action (mcts.py:269-306) for every tree with exactly num_sims
 * simulations each (the time-bounded loop of mcts.py:285 becomes a count).
 * actions_out (host, [num_trees]) may be NULL: results stay on device. */
int pomcp_search(pomcp_ctx* ctx, int32_t num_sims, int32_t* actions_out);
/* num_sims more simulations WITHOUT the final action choice (mcts.py:299-306):
 * a get_action split over several launches -- the wall-clock loop of
 * mcts.py:285 -- is pomcp_search_continue(n1), ..., (nk) then
 * pomcp_search(ctx, 0, ...), and consumes exactly the draws of one
 * pomcp_search(n1 + ... + nk).  Root stats' action is -1 after it. */
int pomcp_search_continue(pomcp_ctx* ctx, int32_t num_sims);

/* Search kernel of pomcp_search / pomcp_search_continue (results are the same
 * bit for bit; only the speed differs):
 *   POMCP_SEARCH_AUTO  (default) wave-per-tree for small batches whose
 *                      scratch fits, tree-per-lane otherwise;
 *   POMCP_SEARCH_LANE  one tree per lane, tree in HBM (k_search: the
 *                      throughput kernel for thousands of trees);
 *   POMCP_SEARCH_WAVE  one wave per tree, tree blocks in LDS (k_search_lds: a
 *                      lone planner's latency, mcts.py:285's loop as fast as one
 *                      tree allows); for depth limits <= 8 the tree's workgroup
 *                      adds step-tree producer waves that evaluate the first
 *                      three levels' generative steps ahead of the search
 *                      (environment POMCP_STEP_TREE=0 / 1 forces them off / on). */
typedef enum pomcp_search_kernel {
  POMCP_SEARCH_AUTO = 0,
  POMCP_SEARCH_LANE = 1,
  POMCP_SEARCH_WAVE = 2
} pomcp_search_kernel;
int pomcp_set_search_kernel(pomcp_ctx* ctx, int32_t kind);
/* The kernel the next search will use (POMCP_SEARCH_LANE or _WAVE). */
int32_t pomcp_search_kernel_used(const pomcp_ctx* ctx);
/* Cut-off children in the lane kernel (k_search): on = 1 (the default) a
 * simulation's arrival at a child beyond the depth / step limits
 * (mcts.py:315) is recorded against its action node and the child is
 * materialised at the next re-root (pomcp_update) -- one slot line less per
 * simulation, the cheaper choice when a tree is searched several times per
 * re-root (batched search throughput); on = 0 looks the child up during the
 * search (as the wave kernel always does) -- the cheaper choice when every
 * search is followed by a re-root (an episode planner).  Same results either
 * way (only node labels differ). */
int pomcp_set_defer_cutoff(pomcp_ctx* ctx, int32_t on);

/* Copy every tree's pomcp_root_stats of the last search to host. */
int pomcp_get_root_stats(pomcp_ctx* ctx, pomcp_root_stats* out);

/* Host particles as the root belief of one FRESH tree (after pomcp_reset,
 * before its first update): `particles` = count (t, v0, v1) u32 triples in
 * insertion order (ParticleBelief, belief.py:47-64), all with the same t >= 1.
 * The root becomes an unexpanded obs node at time t holding them -- what
 * _initial_update builds (mcts.py:175-227), from the caller's particles
 * instead of b0 samples (no RNG draws).  Searches and updates follow as usual. */
int pomcp_set_root_belief(pomcp_ctx* ctx, int32_t tree, const uint32_t* particles, int32_t count);

/* Root belief particles of one tree as (t, v0, v1) u32 triples (belief.py:47-64). */
int pomcp_get_root_belief(pomcp_ctx* ctx, int32_t tree, uint32_t* out, int32_t capacity,
                          int32_t* count);

/* POTMMCP (potmmcp.py:18-301) with non-neural policies: a context created with
 * pomcp_config.type_based = 1 searches with a meta-policy over the ego's
 * policies and a mixture over the other agent's policies, every policy a fixed
 * action distribution (planning/policies.py FixedDistributionPolicy):
 *   - the root belief's particles carry the other agent's policy, drawn by
 *     OtherAgentMixturePolicy.sample_initial_state (other_policy.py:178-183);
 *   - every simulation draws an ego policy from the meta-policy row of its
 *     particle's other-agent policy (POTMMCPMetaPolicy.sample_policy,
 *     potmmcp.py:381-389); the ego rolls out with it (potmmcp.py:221-229) and
 *     the other agent acts by its particle's policy;
 *   - every obs node keeps ObsNode.action_probs, PUCB's prior (mcts.py:492-527):
 *     a child created by a simulation starts with that simulation's ego policy
 *     distribution, a root made by update with `expected_prior`
 *     (get_expected_action_probs(None, ...), potmmcp.py:391-431), and a node's
 *     priors move towards the simulation's policy on every arrival at an
 *     existing child (potmmcp.py:255-264).
 * Draws follow CPython's random.choices (cumulative weights, bisection).  Must
 * be called after pomcp_create and before the first update. */
typedef struct pomcp_type_policies {
  int32_t num_ego;                 /* POTMMCPMetaPolicy.policies, 1..8 */
  int32_t num_other;               /* OtherAgentMixturePolicy.policies, 1..8 (dict order) */
  double ego_pi[POMCP_MAX_TYPE_POLICIES][POMCP_MAX_ACTIONS];     /* get_pi, action order */
  double other_pi[POMCP_MAX_TYPE_POLICIES][POMCP_MAX_ACTIONS];
  /* meta_policy[other policy j]: its keys (ego policy indices) and weights in the dict's order */
  int32_t meta_len[POMCP_MAX_TYPE_POLICIES];
  int32_t meta_policy[POMCP_MAX_TYPE_POLICIES][POMCP_MAX_TYPE_POLICIES];
  double meta_weight[POMCP_MAX_TYPE_POLICIES][POMCP_MAX_TYPE_POLICIES];
  double expected_prior[POMCP_MAX_ACTIONS];
  /* The base planner (MCTS / IPOMCP / POMCP, mcts.py:22-739) with fixed-
   * distribution policies runs on the same machinery; zeros = POTMMCP:
   *   no_meta_draw     no sample_policy draw per simulation (ego policy 0 = the
   *                    search policy, potmmcp.py:381-389 is POTMMCP's only);
   *   no_mixture_draw  no policy draw per initial particle (the other agent is
   *                    one stateless policy, index 0: state_belief_only=True);
   *   ego_uniform      the ego's rollout draws Discrete.sample() (RandomSearchPolicy,
   *                    search_policy.py:170) instead of random.choices over ego_pi;
   *   other_uniform    the other agent draws Discrete.sample()
   *                    (RandomOtherAgentPolicy, other_policy.py:151). */
  int32_t no_meta_draw, no_mixture_draw, ego_uniform, other_uniform;
} pomcp_type_policies;
int pomcp_set_type_policies(pomcp_ctx* ctx, const pomcp_type_policies* tp);

/* Type-based contexts: the root's ObsNode.action_probs (num_actions doubles) and
 * its particles' other-agent policy indices (belief order). */
int pomcp_get_root_prior(pomcp_ctx* ctx, int32_t tree, double* out);
int pomcp_get_root_policies(pomcp_ctx* ctx, int32_t tree, int32_t* out, int32_t capacity,
                            int32_t* count);

/* Belief accuracy counts of every tree's current root belief, reduced on the
 * device (k_belief_stats): what BeliefStatTracker (utils.py:147-339) needs of
 * planner.root.belief without copying a particle to the host.
 *   belief_size    planner.root.belief.size() (utils.py:227-228);
 *   state_matches  particles whose state words (v0, v1) equal the tree's query
 *                  state (get_state_accuracy, utils.py:292-297: hps.state ==
 *                  state; the particle's t is not compared), -1 without states;
 *   policy_hist[j] particles whose other-agent policy is index j (dict order of
 *                  OtherAgentMixturePolicy.policies): the operand of
 *                  get_other_policy_accuracy (utils.py:309-324) and
 *                  get_other_action_accuracy (utils.py:326-339).  Type-based
 *                  contexts only; zeros on plain contexts, whose particles
 *                  carry no policy;
 *   error          the tree's pomcp_status, or POMCP_E_INVALID if a particle's
 *                  policy index is out of range (it is then in no bin). */
typedef struct pomcp_belief_counts {
  int32_t belief_size, state_matches, error, pad;
  int32_t policy_hist[POMCP_MAX_TYPE_POLICIES];
} pomcp_belief_counts;
/* states: host [num_trees][2] (v0, v1) or NULL (state_matches = -1).  out: host
 * [num_trees].  Runs on the context stream, after the update / search before
 * it (a search leaves the root belief as it is).  POMCP_E_STATE before the
 * first update (or pomcp_set_root_belief) after a reset, POMCP_E_INVALID on a
 * null ctx / out; a tree's non-zero error is returned after `out` is filled. */
int pomcp_belief_stats(pomcp_ctx* ctx, const uint32_t* states, pomcp_belief_counts* out);

/* Arena use: the largest block count and particle-log record count over the
 * trees (after the last update's subtree compaction / the last search).  The
 * wall-clock loop sizes its chunks from it (never overflowing the arenas). */
int pomcp_arena_usage(pomcp_ctx* ctx, int32_t* max_blocks_used, int32_t* max_log_used);

/* Root-parallel search: re-key every tree's streams to `seed`
 * keeping counters (rank g uses seed ^ (g << 32)). */
int pomcp_rekey(pomcp_ctx* ctx, uint64_t seed);

/* Exchange record of one tree, written by pomcp_search (the operand of the
 * root-parallel exchange at action-selection time): POMCP_XREC(A) doubles =
 *   [2a] child visits, [2a + 1] child total value    (a < num_actions)
 *   [2A + 0] num_sims, [2A + 1] root visits, [2A + 2] search depth,
 *   [2A + 3] error (pomcp_status), [2A + 4] min value, [2A + 5] max value
 * (integers are exact in a double). */
#define POMCP_XREC_STATS 6
#define POMCP_XREC(num_actions) (2 * (num_actions) + POMCP_XREC_STATS)

/* Device pointer of the merge buffer: double[num_trees][POMCP_XREC(A)], this
 * GPU's exchange records. */
int pomcp_root_merge_buffer(pomcp_ctx* ctx, void** device_ptr);

/* Device pointer of the gather buffer: double[world][num_trees][POMCP_XREC(A)],
 * every rank's merge buffer in rank order (allocated on the first call for a
 * given world size; a larger world re-allocates).  The caller may fill it with
 * its own all-gather (e.g. torch.distributed.all_gather_into_tensor) instead
 * of pomcp_allgather_root. */
int pomcp_root_gather_buffer(pomcp_ctx* ctx, int32_t world, void** device_ptr);

/* The root-parallel exchange of SURVEY §8(b)/(e) (mcts.py:269-306 run as
 * root-parallel trees on several GPUs): ncclAllGather(merge buffer -> gather
 * buffer, num_trees * POMCP_XREC(A) doubles per rank, comm, context stream),
 * before pomcp_merge_roots(..., world, ...).  An all-gather, not an
 * all-reduce: the merge then sums the replicas in one fixed order on every
 * rank (a ring all-reduce's summation order depends on the algorithm and the
 * rank count, so its FP64 sums could not be restated).  rccl_comm: an
 * ncclComm_t of `world` ranks, one per GPU, created by the RCCL library that
 * is already loaded in this process (PyTorch's, or one the caller loaded): the
 * library never loads a second RCCL copy; POMCP_E_UNSUPPORTED if none is loaded. */
int pomcp_allgather_root(pomcp_ctx* ctx, void* rccl_comm, int32_t world);

/* Root-parallel decision of one planner. */
typedef struct pomcp_merged_root {
  int32_t action;               /* merged final action (see pomcp_merge_roots) */
  int32_t num_trees;            /* replicas merged */
  int32_t search_depth;         /* max over the replicas */
  int32_t error;                /* first non-zero replica error, in replica order */
  int64_t num_sims;             /* summed over the replicas */
  int64_t root_visits;          /* summed */
  double min_value, max_value;  /* min / max over the replicas' MinMaxStats */
  double visits[POMCP_MAX_ACTIONS];   /* summed root child visits */
  double totals[POMCP_MAX_ACTIONS];   /* summed root child total values */
} pomcp_merged_root;

/* Root-parallel merge on the device: trees [g*group, (g+1)*group) are the
 * replicas of planner g on every rank (num_trees % group == 0).
 *   world == 0: this GPU's merge buffer alone (replicas k = 0..group-1);
 *   world >= 1: the gather buffer of `world` ranks (pomcp_allgather_root):
 *               replica j = r * group + k is tree g*group + k of rank r.
 * Replica records are summed in one fixed order -- lane l of a 64-lane wave
 * sums replicas [l*c, (l+1)*c), c = ceil(N / 64), N = max(world,1) * group, in
 * replica order from 0.0, then the 64 partials in lane order from 0.0
 * (restated by oracle/root_parallel.py) -- so every rank takes the same
 * decision, bit-identical to one GPU merging all N replicas:
 *   PUCB: argmax summed visits (the merged max_visit_action_selection,
 *         mcts.py:565-581);  UCB / uniform: argmax summed total / summed visits
 *         over visited actions (max_value_action_selection, mcts.py:583-600);
 * lowest action on ties, 0 if nothing was visited.  Replaces the reference's
 * single-tree _final_action_selection when one planner runs many trees.
 * out (host, [num_trees / group]) may be NULL: the result stays on device. */
int pomcp_merge_roots(pomcp_ctx* ctx, int32_t group, int32_t world, pomcp_merged_root* out);

/* Bench / batch helpers: synthetic roots (the configured environment).  Tree b samples s0 from
 * the model's b0 under env key (env_seed_base + b, 0x40000000) and the ego's
 * initial obs is written to obs_keys_out (host, [num_trees], may be NULL). */
int pomcp_synthetic_obs(pomcp_ctx* ctx, uint64_t env_seed_base, uint64_t* obs_keys_out);
/* The environment's answer to the planners' actions (env.step of the episode
 * loop, exp_utils.py:481-505, for the synthetic roots): tree b's true initial
 * state (as pomcp_synthetic_obs) stepped with actions[b] (host, [num_trees]) and
 * the other agent's uniformly drawn action (env key's action stream); the ego's
 * next observation -> obs_keys_out (host, may be NULL).  For update()-inclusive
 * benchmark steps. */
int pomcp_synthetic_step(pomcp_ctx* ctx, uint64_t env_seed_base, const int32_t* actions,
                         uint64_t* obs_keys_out);
/* Save / restore the complete post-update root state (headers, root nodes,
 * root belief, RNG counters) so a timed loop can re-search the same roots. */
int pomcp_snapshot(pomcp_ctx* ctx);
int pomcp_restore(pomcp_ctx* ctx);

/* ---- Host (CPU) Driving-v1 model from the same header (driving.h) -------
 * The environment side of the episode loop (env.step in
 * tests/planning/test_pomcp.py:23-29); not on the planner's hot path. */
int pomcp_driving_sample_initial_state(const pomcp_grid* g, uint64_t seed, uint32_t tree,
                                       uint32_t* model_ctr, uint32_t state_out[2]);
/* One joint step; draws the execution-order shuffle from the model stream
 * (seed, tree) at counter *model_ctr (advanced). */
int pomcp_driving_step(const pomcp_grid* g, uint64_t seed, uint32_t tree, uint32_t* model_ctr,
                       const uint32_t state[2], const int32_t actions[2], uint32_t next_out[2],
                       double rewards_out[2], int32_t terminated_out[2],
                       uint64_t obs_keys_out[2]);
int pomcp_driving_obs(const pomcp_grid* g, const uint32_t state[2], uint64_t obs_keys_out[2]);

/* ---- Host (CPU) PursuitEvasion-v1 model from csrc/pursuit_evasion.h ----- */
int pomcp_pe_sample_initial_state(const pomcp_pe_grid* g, uint64_t seed, uint32_t tree,
                                  uint32_t* model_ctr, uint32_t state_out[2]);
/* One joint step (deterministic: no model draw). */
int pomcp_pe_step(const pomcp_pe_grid* g, const uint32_t state[2], const int32_t actions[2],
                  uint32_t next_out[2], double rewards_out[2], int32_t terminated_out[2],
                  uint64_t obs_keys_out[2]);
int pomcp_pe_obs(const pomcp_pe_grid* g, const uint32_t state[2], uint64_t obs_keys_out[2]);

/* ---- Host (CPU) CooperativeReaching-v0 model from csrc/cooperative_reaching.h */
int pomcp_cr_sample_initial_state(const pomcp_cr_grid* g, uint64_t seed, uint32_t tree,
                                  uint32_t* model_ctr, uint32_t state_out[2]);
/* One joint step (deterministic: no model draw). */
int pomcp_cr_step(const pomcp_cr_grid* g, const uint32_t state[2], const int32_t actions[2],
                  uint32_t next_out[2], double rewards_out[2], int32_t terminated_out[2],
                  uint64_t obs_keys_out[2]);
int pomcp_cr_obs(const pomcp_cr_grid* g, const uint32_t state[2], uint64_t obs_keys_out[2]);
/* model.sample_agent_initial_state(agent, obs) with the model stream at
 * *model_ctr; POMCP_E_INVALID for an observation outside the model. */
int pomcp_cr_sample_agent_initial_state(const pomcp_cr_grid* g, int32_t agent, uint64_t obs_key,
                                        uint64_t seed, uint32_t tree, uint32_t* model_ctr,
                                        uint32_t state_out[2]);

/* ---- Host (CPU) PredatorPrey-v0 model from csrc/predator_prey.h */
int pomcp_pp_sample_initial_state(const pomcp_pp_grid* g, uint64_t seed, uint32_t tree,
                                  uint32_t* model_ctr, uint32_t state_out[2]);
/* One joint step: one draw in [0, 2^25) of the model stream at *model_ctr (the
 * prey's tie bytes and the predators' order). */
int pomcp_pp_step(const pomcp_pp_grid* g, const uint32_t state[2], const int32_t actions[2],
                  uint64_t seed, uint32_t tree, uint32_t* model_ctr, uint32_t next_out[2],
                  double rewards_out[2], int32_t terminated_out[2], uint64_t obs_keys_out[2]);
int pomcp_pp_obs(const pomcp_pp_grid* g, const uint32_t state[2], uint64_t obs_keys_out[2]);
/* model.sample_agent_initial_state(agent, obs) with the model stream at
 * *model_ctr; POMCP_E_INVALID for an observation outside the model. */
int pomcp_pp_sample_agent_initial_state(const pomcp_pp_grid* g, int32_t agent, uint64_t obs_key,
                                        uint64_t seed, uint32_t tree, uint32_t* model_ctr,
                                        uint32_t state_out[2]);
/* ---- Host RNG streams (csrc/philox.h) -----------------------------------
 * out[k] = word (first + k) of Philox stream `stream` under key (seed, tree):
 * the draws of the episode loop's non-planning agents (the reference's
 * UniformOtherAgentFn / Random-v0 policies, baseline_exps/exp_utils.py:481). */
int pomcp_philox_words(uint64_t seed, uint32_t tree, uint32_t stream, uint32_t first, int32_t n,
                       uint32_t* out);

/* ---- Host math.log table -------------------------------------------------
 * out[k] = log(first + k) with the host C library's log (the function
 * Python's math.log calls: mcts.py:534's log(N) bit for bit), 0.0 for 0; the
 * planner's pomcp_config.log_table at C speed (wall-clock arenas ask for tens
 * of millions of entries). */
int pomcp_host_log_table(int64_t first, int64_t n, double* out);

/* ---- Host twin of pomcp_belief_stats ---------------------------------------
 * The counts of one belief given as n host records {t, v0, v1, aux} (4 u32
 * each), with the classification the kernel uses (csrc/belief_stats.h;
 * utils.py:292-339).  state: the query (v0, v1) or NULL (state_matches = -1);
 * num_other: 0 for a plain belief (aux is not read, the histogram stays
 * zero), else the number of other-agent policies (1..8).  An aux >= num_other
 * is counted in no bin: out is filled, out->error = POMCP_E_INVALID and that
 * is returned (as for bad arguments, which leave out untouched). */
int pomcp_host_belief_counts(const uint32_t* records4, int64_t n, const uint32_t* state,
                             int32_t num_other, pomcp_belief_counts* out);

/* ---- Batched episodes on the device (csrc/pomcp_episode.hip) ----------------
 * One episode per tree, played without a host copy of any tree's state: the
 * true environment state, the env streams' counters and the episode's result
 * row live in device memory (run_planning_exp, baseline_exps/exp_utils.py:
 * 468-552, for the whole batch; the other agent is uniform random,
 * exp_utils.py:481, or drawn from a population: pomcp_episodes_set_population
 * below).  A finished tree is parked: it is not searched, re-rooted
 * or reinvigorated again and its record and last root statistics stay as they
 * were, while its neighbours play on. */
typedef enum pomcp_episode_until {
  POMCP_UNTIL_AGENT_DONE = 0,   /* exp_utils.py:522: the planning agent is done */
  POMCP_UNTIL_ALL_DONE = 1      /* tests/planning/test_pomcp.py:28: every agent is */
} pomcp_episode_until;

/* One tree's episode row (exp_utils.py:506-535) and planner statistics. */
typedef struct pomcp_episode_result {
  uint64_t env_seed;
  int32_t len;                   /* environment steps played */
  int32_t searched_steps;        /* steps that reached the planner's statistics: the root was
                                    not absorbing before the step (mcts.py:97-117) */
  double ret;                    /* sum of the ego's rewards, one FP64 add per step */
  double discounted_return;      /* += pow_table[len] * reward, in step order */
  int32_t ego_terminated, all_done, truncated;   /* after the last step played */
  int32_t error;                 /* the tree's pomcp_status */
  int64_t search_depth_sum;      /* over the searched steps */
  int64_t num_sims_sum;
  double min_value_sum;          /* sequential FP64 sums over the searched steps */
  double max_value_sum;
} pomcp_episode_result;

/* One tree's whole episode record (device memory owned by the context; the
 * host twin works on the same struct). */
typedef struct pomcp_episode_state {
  pomcp_episode_result res;
  uint32_t v0, v1;               /* the true joint state */
  uint32_t model_ctr;            /* env model stream: draws consumed */
  uint32_t policy_ctr;           /* the other agent's policy stream: draws consumed */
  int32_t last_action;           /* the ego's last action (-1 before the first step) */
  int32_t finished;              /* by the `until` mode or truncation (or an error) */
  int32_t root_absorbing;        /* the planner's root after the last step's update */
  int32_t last_other_action;     /* the other agent's last action (-1 before the first step) */
  double last_reward;            /* the ego's reward of the last step played */
} pomcp_episode_state;

/* What one step reads of the planner (the tree header and pomcp_root_stats). */
typedef struct pomcp_episode_step_in {
  int32_t root_absorbing;        /* the root after this step's update */
  int32_t action;                /* pomcp_root_stats.action of this step's search */
  int32_t search_depth, num_sims;
  int32_t error, pad;
  double min_value, max_value;
} pomcp_episode_step_in;

typedef struct pomcp_episode_step_out {
  uint64_t obs_key;              /* the ego's next observation */
  double reward;                 /* the ego's reward */
  int32_t ego_action, other_action;
  int32_t stepped, pad;          /* 0: the episode was finished already (nothing changed) */
} pomcp_episode_step_out;

/* pomcp_reset, then every tree's episode starts (k_episode_reset): tree b draws
 * its initial state from the model stream under key (env_seeds[b], 0x40000000)
 * as pomcp_driving_sample_initial_state / pomcp_pe_sample_initial_state do; the
 * ego's initial observation and action -1 become the next update's inputs.
 * pow_table: max_steps doubles, pow_table[t] = discount ** t as the host's
 * Python computes it (the serial harness's `gamma ** len`, libm's pow).
 * until: pomcp_episode_until. */
int pomcp_episodes_begin(pomcp_ctx* ctx, const uint64_t* env_seeds, const double* pow_table,
                         int32_t max_steps, int32_t until);
/* One episode step of every unfinished tree, with nothing per tree on the
 * host: update from the device inputs (re-root unless this is the batch's first
 * step), search with num_sims, k_episode_step (the environment's answer, the
 * result row, the next update's inputs, finished trees parked).  live_out: the
 * number of unfinished trees afterwards.  Tree errors surface as they do from
 * pomcp_update / pomcp_search. */
int pomcp_episodes_step(pomcp_ctx* ctx, int32_t num_sims, int32_t* live_out);
/* Every tree's row (host, [num_trees]). */
int pomcp_episodes_results(pomcp_ctx* ctx, pomcp_episode_result* out);
/* Every tree's whole record (host, [num_trees]): tests and diagnostics. */
int pomcp_episodes_states(pomcp_ctx* ctx, pomcp_episode_state* out);
/* on = 1: k_episode_reset / k_episode_step also write the true state the root
 * belief is about -- the state before the step's joint action, (v0, v1) --
 * into the query-state buffer of pomcp_belief_stats, and
 * pomcp_episodes_belief_stats counts every root belief against it with no host
 * copy of a state.  A finished tree keeps its last entry.  Takes effect at the
 * next pomcp_episodes_begin. */
int pomcp_episodes_track_states(pomcp_ctx* ctx, int32_t on);
int pomcp_episodes_belief_stats(pomcp_ctx* ctx, pomcp_belief_counts* out);
/* Device time (ms, events on the context stream) since pomcp_episodes_begin:
 * ms[0] updates, ms[1] searches, ms[2] k_episode_step + the live count;
 * *steps = pomcp_episodes_step calls. */
int pomcp_episodes_timing(pomcp_ctx* ctx, double ms[3], int32_t* steps);

/* ---- Host twin of the per-tree episode step (csrc/episode_step.h) ----------
 * The code k_episode_reset / k_episode_step run per tree, on the host.
 * grid: a pomcp_grid (env_id POMCP_ENV_DRIVING), a pomcp_pe_grid, a
 * pomcp_cr_grid (POMCP_ENV_COOPERATIVE_REACHING) or a pomcp_pp_grid
 * (POMCP_ENV_PREDATOR_PREY). */
int pomcp_host_episode_reset(int32_t env_id, const void* grid, int32_t ego, uint64_t env_seed,
                             pomcp_episode_state* st, uint64_t* obs_key_out);
int pomcp_host_episode_step(int32_t env_id, const void* grid, int32_t ego,
                            const pomcp_episode_step_in* in, const double* pow_table,
                            int32_t max_steps, int32_t until, pomcp_episode_state* st,
                            pomcp_episode_step_out* out);

/* ---- Batched episodes against a policy population (ABI 7, additive) ----------
 * The other agent of every episode is drawn from a test population of fixed
 * action distributions (UniformOtherAgentFn, utils/agent_env_wrapper.py:8-27:
 * model.rng.choice(ids) at every reset; run_planning_exp,
 * baseline_exps/exp_utils.py:468-552).  Tree b plays policy
 *   uniform_int(word 0 of stream 44 under key (env_seeds[b], 0x40000000), num_policies)
 * and that policy draws its action from word j of the other agent's policy
 * stream (40 + agent) at its step j as CPython's random.choices does:
 * bisect_right(cumulative(pi), word * 2^-32 * total, 0, A - 1). */
typedef struct pomcp_episode_population {
  int32_t num_policies;          /* 1..POMCP_MAX_TYPE_POLICIES */
  int32_t pad;
  double pi[POMCP_MAX_TYPE_POLICIES][POMCP_MAX_ACTIONS];   /* get_pi, action order */
  /* index of the policy's id in the planner's OtherAgentMixturePolicy.policies
   * (pomcp_type_policies.other_pi's order), -1: the planner does not model it */
  int32_t mixture_index[POMCP_MAX_TYPE_POLICIES];
} pomcp_episode_population;

/* One tree's population record (a device array of its own, beside the
 * pomcp_episode_state records). */
typedef struct pomcp_episode_pop_state {
  int32_t policy_index;          /* the episode's policy, -1 without a population */
  int32_t mixture_index;         /* its pomcp_episode_population.mixture_index, else -1 */
} pomcp_episode_pop_state;

/* The population of the batches started by the following pomcp_episodes_begin
 * calls (copied); NULL: back to the uniform random other agent. */
int pomcp_episodes_set_population(pomcp_ctx* ctx, const pomcp_episode_population* pop);
/* Every tree's population record (host, [num_trees]). */
int pomcp_episodes_pop_states(pomcp_ctx* ctx, pomcp_episode_pop_state* out);

/* Belief accuracy accumulated on the device (k_episode_belief_acc): after
 * k_episode_step, every tree that played this step adds the accuracies of its
 * root belief (BeliefStatTracker.step, utils.py:147-339) to its record, in
 * FP64 without contraction:
 *   state   matches / n against the state before the joint action;
 *   policy  hist[mixture_index of the tree's true policy] / n (0.0 for -1);
 *   action  (sum over j ascending, hist[j] != 0, of hist[j] * other_pi[j][a]) / n
 *           with a the other agent's action of this step and other_pi the
 *           planner's pomcp_type_policies.other_pi;
 * all 0.0 for an empty belief; policy and action 0.0 when the particles carry
 * no policy (a plain context, or no_mixture_draw).  A parked tree is skipped
 * without a particle of it being read: its record stays as it is. */
typedef struct pomcp_episode_belief_acc {
  double state_sum, policy_sum, action_sum;   /* sequential sums over the steps played */
  int32_t count;                 /* steps recorded (= pomcp_episode_result.len) */
  int32_t error;                 /* the tree's pomcp_status; POMCP_E_INVALID: a particle's
                                    policy index out of range */
} pomcp_episode_belief_acc;
/* on = 1: from the next pomcp_episodes_begin on (implies
 * pomcp_episodes_track_states); per_step = 1 also keeps every step's three
 * values.  A record's error surfaces from pomcp_episodes_step. */
int pomcp_episodes_track_belief_acc(pomcp_ctx* ctx, int32_t on, int32_t per_step);
/* Every tree's record (host, [num_trees]). */
int pomcp_episodes_belief_acc(pomcp_ctx* ctx, pomcp_episode_belief_acc* out);
/* The per-step table (host, [num_trees][max_steps][3] doubles: state, policy,
 * action; entries at t >= count are unspecified).  POMCP_E_STATE without per_step. */
int pomcp_episodes_belief_acc_steps(pomcp_ctx* ctx, double* out);
/* Device time (ms) of k_episode_belief_acc since pomcp_episodes_begin. */
int pomcp_episodes_belief_acc_ms(pomcp_ctx* ctx, double* ms);

/* Host twins: episode_step.h's population overloads (pop NULL: exactly
 * pomcp_host_episode_reset / _step; ps may then be NULL) and the accuracy
 * arithmetic k_episode_belief_acc does on a tree's counts (belief_stats.h
 * bel_accuracy).  other_pi: the planner's [num_other][POMCP_MAX_ACTIONS] table
 * (may be NULL when num_other = 0); out = {state, policy, action}. */
int pomcp_host_episode_reset_pop(int32_t env_id, const void* grid, int32_t ego, uint64_t env_seed,
                                 const pomcp_episode_population* pop, pomcp_episode_state* st,
                                 pomcp_episode_pop_state* ps, uint64_t* obs_key_out);
int pomcp_host_episode_step_pop(int32_t env_id, const void* grid, int32_t ego,
                                const pomcp_episode_step_in* in, const double* pow_table,
                                int32_t max_steps, int32_t until,
                                const pomcp_episode_population* pop,
                                const pomcp_episode_pop_state* ps, pomcp_episode_state* st,
                                pomcp_episode_step_out* out);
int pomcp_host_belief_acc(const pomcp_belief_counts* counts, int32_t mixture_index,
                          int32_t other_action, const double* other_pi, int32_t num_other,
                          double out[3]);

/* ---- State-reactive population policies (ABI 7, additive) --------------------
 * A policy of the population may act on the true state instead of drawing from
 * a fixed distribution.  POMCP_POLICY_DRIVING_SHORTEST_PATH is the Driving-v1
 * shortest-path agent (csrc/driving_policy.h drv_sp_action; the registry ids
 * Driving-v1/A{0,40,60,80,100}Shortestpath-v0 of planning/policies.py):
 *   param0  caution, 0..15: the rows of its observation window ahead in which
 *           another vehicle makes it brake;
 *   param1  vmax, 0..3: the speed it does not exceed while it has a choice.
 * Its action is a function of the state before the joint action.  The word of
 * the agent's policy stream is still taken at every step, so every counter
 * advances as with a fixed distribution; the policy's pi row is not read (it
 * must still be a valid distribution).
 * POMCP_POLICY_CR_GOAL is the CooperativeReaching-v0 heuristic agent
 * (csrc/cooperative_reaching.h cr_goal_action; the registry ids
 * CooperativeReaching-v0/H{1..5}-v0): param0 is the rule 0..4 that picks its
 * target goal from its start cell, param1 must be 0.
 * POMCP_POLICY_PP_HEURISTIC is the PredatorPrey-v0 heuristic agent
 * (csrc/predator_prey_policy.h; the registry ids PredatorPrey-v0/H{1,2,3}-v0):
 * param0 is the rule 0..2 that picks its target (the nearest prey it sees; the
 * other predator first; the prey the other predator is nearest to), param1 must
 * be 0.  It is a STOCHASTIC reactive kind: the rule gives a distribution over up
 * to four moves that depends on the state, and the word of the agent's stream,
 * which the deterministic kinds take and ignore, picks from it as
 * random.choices does from a fixed row.  (Kinds 2 and 4 are unassigned.) */
enum {
  POMCP_POLICY_FIXED = 0,
  POMCP_POLICY_DRIVING_SHORTEST_PATH = 1,
  POMCP_POLICY_CR_GOAL = 3,
  POMCP_POLICY_PP_HEURISTIC = 5
};
typedef struct pomcp_policy_kinds {
  int32_t kind[POMCP_MAX_TYPE_POLICIES];
  int32_t param0[POMCP_MAX_TYPE_POLICIES];
  int32_t param1[POMCP_MAX_TYPE_POLICIES];
} pomcp_policy_kinds;
/* The kinds of the population set last (copied; entries past its num_policies
 * are not read); NULL: all fixed, which is also what every
 * pomcp_episodes_set_population leaves.  POMCP_E_STATE without a population,
 * POMCP_E_UNSUPPORTED for a reactive kind the context's environment does not have,
 * POMCP_E_INVALID for an unknown kind or a parameter out of range. */
int pomcp_episodes_set_population_kinds(pomcp_ctx* ctx, const pomcp_policy_kinds* kinds);
/* The kinds of a type-based context's other-agent policies (other_pi's order),
 * valid after pomcp_set_type_policies, which resets them to fixed: a particle
 * whose policy is reactive has the other agent act on the simulated state in
 * the tree levels, the rollouts and the rejection reinvigoration.  The word of
 * the action stream is still taken.  NULL: all fixed.  POMCP_E_STATE before
 * pomcp_set_type_policies, POMCP_E_UNSUPPORTED for a reactive kind the context's
 * environment does not have, POMCP_E_INVALID for a bad kind or parameter or with
 * other_uniform. */
int pomcp_set_type_policy_kinds(pomcp_ctx* ctx, const pomcp_policy_kinds* kinds);
/* The kinds of a type-based context's EGO policies (ego_pi's order), valid after
 * pomcp_set_type_policies, which resets them to fixed.  A reactive ego policy
 * acts on the simulated state wherever the search reads an ego policy: the
 * rollout action (the word of the ego's action stream is still taken), the
 * prior of a node created under it (one-hot on its action at that node), the
 * moving average of a node's prior, and the expected prior of a root made by
 * pomcp_update, sum_k expected_meta[k] * pi_k(root) normalised by its sum.
 * expected_meta: num_ego doubles, the normalised expected meta-policy in
 * ego_pi's order (potmmcp.py:391-420 with a uniform prior over the other
 * agent's policies); read only when some kind is reactive.  The ego_pi row of
 * a reactive policy and expected_prior are then not read (they must still be
 * valid).  Only POMCP_POLICY_CR_GOAL on a CooperativeReaching-v0 context is an
 * ego kind: the policy must be a function of the ego's own state word at every
 * node.  NULL kinds: all fixed.  POMCP_E_STATE before
 * pomcp_set_type_policies, POMCP_E_UNSUPPORTED for a reactive kind on another
 * environment, POMCP_E_INVALID for a bad kind, parameter or weight, or with
 * ego_uniform.  pomcp_get_root_prior of a root that has no block yet builds
 * the line from a root particle (POMCP_E_STATE when it has none). */
int pomcp_set_type_ego_kinds(pomcp_ctx* ctx, const pomcp_policy_kinds* kinds,
                             const double* expected_meta);
/* Host twin of the prior line k_search writes under reactive ego policies
 * (csrc/tm_prior.h): out[i][0 .. 5) for prior code `code` (0: the expected
 * prior, k + 1: ego policy k's) at the ego word own[i] on a CooperativeReaching
 * grid.  ego_pi: [num_ego][POMCP_MAX_ACTIONS]; expected_prior: 5 doubles, the
 * code-0 line when no kind is reactive. */
int pomcp_host_cr_prior_lines(const pomcp_cr_grid* grid, int32_t num_ego, const double* ego_pi,
                              const double* expected_prior, const pomcp_policy_kinds* kinds,
                              const double* expected_meta, int32_t code, int64_t n,
                              const uint32_t* own, double* out);

/* Host twins.  out[i] = drv_sp_action(grid, own[i], other[i], caution, vmax)
 * for n pairs of packed vehicle words. */
int pomcp_host_driving_policy_actions(const pomcp_grid* grid, int64_t n, const uint32_t* own,
                                      const uint32_t* other, int32_t caution, int32_t vmax,
                                      int32_t* out);
/* out[i] = cr_goal_action(grid, own[i], rule) for n packed agent words (the
 * rule never reads the other agent's word). */
int pomcp_host_cr_policy_actions(const pomcp_cr_grid* grid, int64_t n, const uint32_t* own,
                                 int32_t rule, int32_t* out);
/* The PredatorPrey-v0 heuristic agents on n states (w0[i], w1[i]) for predator
 * `agent` under rule 0..2: out[i][0 .. 5) = the rule's action distribution, and
 * out[i] = the action the word words[i] of the agent's stream draws from it
 * (random.choices' bisection of the cumulative weights).  POMCP_E_INVALID: a
 * null pointer, n < 0, a grid this build does not restate, agent not 0 / 1 or
 * a bad rule. */
int pomcp_host_pp_policy_pi(const pomcp_pp_grid* grid, int64_t n, const uint32_t* w0,
                            const uint32_t* w1, int32_t agent, int32_t rule, double* out);
int pomcp_host_pp_policy_actions(const pomcp_pp_grid* grid, int64_t n, const uint32_t* w0,
                                 const uint32_t* w1, int32_t agent, int32_t rule,
                                 const uint32_t* words, int32_t* out);
/* pomcp_host_episode_step_pop with the population's kinds (NULL: exactly that
 * call). */
int pomcp_host_episode_step_pop_kinds(int32_t env_id, const void* grid, int32_t ego,
                                      const pomcp_episode_step_in* in, const double* pow_table,
                                      int32_t max_steps, int32_t until,
                                      const pomcp_episode_population* pop,
                                      const pomcp_policy_kinds* kinds,
                                      const pomcp_episode_pop_state* ps, pomcp_episode_state* st,
                                      pomcp_episode_step_out* out);

/* ---- Episode queue (ABI 7, additive; csrc/pomcp_episode_queue.hip) ----------
 * n >= num_trees episodes on the context's num_trees slots: a tree whose
 * episode ends takes the next environment seed of a device-resident queue
 * instead of staying parked.  The assignment rule: slot b starts with entry b
 * and next = num_trees; at the end of each pomcp_episodes_step the slots whose
 * episode finished in that step take entries next, next + 1, ... in ascending
 * slot order while entries remain; a slot that finds the queue empty is retired
 * (parked as a finished tree is, its last real search's root statistics kept).
 * A refilled tree is reset as pomcp_reset resets it (its RNG stream counters
 * carry on, as over planner.reset() in the serial harness) and its records
 * leave its search wave's shared particle log (k_log_drop) while the wave's
 * other trees are mid-episode. */
typedef struct pomcp_episode_queue_row {
  pomcp_episode_result res;      /* the episode's row */
  int32_t slot;                  /* the tree that played it */
  int32_t slot_order;            /* its ordinal among that tree's episodes */
  int32_t policy_index;          /* pomcp_episode_pop_state.policy_index of the episode */
  int32_t start_step;            /* the pomcp_episodes_step call (from 0) it started at */
  pomcp_episode_belief_acc acc;  /* zero unless pomcp_episodes_track_belief_acc */
} pomcp_episode_queue_row;

/* pomcp_episodes_begin on env_seeds[0 .. num_trees), then queue mode: env_seeds
 * has n >= num_trees entries (copied).  pomcp_episodes_begin and pomcp_reset end
 * queue mode.  The per-step accuracy table is not kept in queue mode. */
int pomcp_episodes_queue_begin(pomcp_ctx* ctx, const uint64_t* env_seeds, int32_t n,
                               const double* pow_table, int32_t max_steps, int32_t until);
/* While a queue is active pomcp_episodes_step also ranks the finished slots,
 * writes their rows, refills or retires them and drops the refilled trees' log
 * records; its live_out is then unfinished + refilled slots (0: every entry
 * has been played). */
/* The rows (host, [n], queue order); the row of an entry that has not finished
 * is zero. */
int pomcp_episodes_queue_rows(pomcp_ctx* ctx, pomcp_episode_queue_row* out);
/* The entry each slot is playing (host, [num_trees]); -1: retired. */
int pomcp_episodes_queue_slots(pomcp_ctx* ctx, int32_t* out);
/* The episodes that ended in the last pomcp_episodes_step (host, [num_trees]
 * each): queue_index_out[b] = the entry that ended in slot b, else -1, and
 * states_out[b] = its whole final record (unspecified for -1) -- the slot's own
 * record is the next episode's by then. */
int pomcp_episodes_queue_finished(pomcp_ctx* ctx, pomcp_episode_state* states_out,
                                  int32_t* queue_index_out);
/* Device time (ms) since pomcp_episodes_queue_begin: ms[0] the rank and refill
 * kernels, ms[1] k_log_drop (both taken out of pomcp_episodes_timing's ms[2]). */
int pomcp_episodes_queue_timing(pomcp_ctx* ctx, double ms[2]);

/* Host twins (csrc/episode_queue.h: the kernels' per-record and per-slot
 * decisions).  pomcp_host_log_drop: k_log_drop on a log given as structure of
 * arrays (aux may be NULL), in place: the records whose tree lane (id >> 26) is
 * in lane_mask leave, the others keep their order; *count_out = records kept.
 * pomcp_host_queue_assign: one step of the assignment rule.  queue_index[b]:
 * the entry slot b plays (-1: retired), finished[b]: its episode record's
 * flag; assign_out[b] = the slot's new entry, -1 (retired now) or -2 (plays
 * on, or was retired before); *next_io is advanced; *refilled_out = slots
 * refilled. */
int pomcp_host_log_drop(uint32_t* ids, uint32_t* v0, uint32_t* v1, uint32_t* aux, int64_t n,
                        uint64_t lane_mask, int64_t* count_out);
int pomcp_host_queue_assign(const int32_t* queue_index, const int32_t* finished,
                            int32_t num_slots, int32_t n, int32_t* next_io, int32_t* assign_out,
                            int32_t* refilled_out);

/* ---- Batched episodes with root-parallel planners (additive;
 * csrc/pomcp_episode_group.hip) -------------------------------------------
 * group = K > 1: the num_trees trees are num_trees / K planners of K replica
 * trees each (planner g owns trees [g*K, (g+1)*K), as pomcp_merge_roots groups
 * them) and every PLANNER plays one episode: after the search the replicas'
 * roots are merged on the device (pomcp_merge_roots' kernel, world = 0), the
 * merged action steps the planner's one environment and every replica is
 * updated with that action and the real observation.  The planner's root is
 * absorbing only when every replica's is; a replica whose own root is
 * absorbing does not search and merges as zeros while its siblings play on; a
 * searched step reports K * num_sims simulations, the merged maximum depth and
 * the merged min / max of the replicas' MinMaxStats; a step whose update made
 * every replica absorbing reports action 0, depth 0 and no simulation.
 *
 * pomcp_episodes_set_group takes effect at the next pomcp_episodes_begin;
 * group >= 1 must divide num_trees (POMCP_E_INVALID otherwise); 1 (the
 * default) is one episode per tree.  With group > 1:
 *   - env_seeds, pomcp_episodes_results, _states and _pop_states have
 *     num_trees / group entries, one per planner;
 *   - pomcp_episodes_step's num_sims is per replica, *live_out counts planners;
 *     pomcp_episodes_timing's ms[1] includes the merge and ms[2] is
 *     k_group_episode_step + the live count;
 *   - a planner's error is the first non-zero error of its replicas in replica
 *     order, the update's before the search's, and surfaces from
 *     pomcp_episodes_step with pomcp_update's / pomcp_search's text;
 *   - pomcp_episodes_begin returns POMCP_E_UNSUPPORTED, before any launch,
 *     with pomcp_episodes_track_states(1) or pomcp_episodes_track_belief_acc(1,
 *     ..) in force, and so does pomcp_episodes_queue_begin;
 *   - the root statistics (pomcp_get_root_stats) of a finished planner's
 *     replicas are unspecified: the searches after the park rewrite them and
 *     the exchange records with zeros.  pomcp_episodes_merged_roots returns
 *     the record that is kept instead: out[g] (host, [num_trees / group]) is
 *     the pomcp_merged_root of planner g's last real step, a step at which its
 *     root was absorbing neither before nor after the update and nothing
 *     failed (zeros before the first one).  POMCP_E_STATE without a running
 *     batch of groups. */
int pomcp_episodes_set_group(pomcp_ctx* ctx, int32_t group);
int pomcp_episodes_merged_roots(pomcp_ctx* ctx, pomcp_merged_root* out);

/* Host twin of the per-group decision (csrc/episode_group.h, the code
 * k_group_episode_step runs): flags = [group][3] {root_absorbing, update error,
 * search error} of the replicas after this step's update and search, merged =
 * their pomcp_merged_root, num_sims = the simulations per replica.  *in_out is
 * the planner's part of the step for pomcp_host_episode_step; *keep_out (may
 * be NULL) = 1 if this is a real step of a planner whose root was not
 * absorbing before it (the merged record is the one to keep). */
int pomcp_host_episode_group_step_in(const int32_t* flags, int32_t group, int32_t num_sims,
                                     const pomcp_merged_root* merged,
                                     pomcp_episode_step_in* in_out, int32_t* keep_out);

/* ---- Episode queue of root-parallel planners (additive;
 * csrc/pomcp_episode_group_queue.hip) --------------------------------------
 * n >= num_trees / group episodes on the num_trees / group PLANNERS of a batch
 * of groups: the queue's slots are the groups (group g = trees [g*group,
 * (g+1)*group)), and the assignment rule is the episode queue's with "slot"
 * meaning "group": group g starts with entry g, the groups whose episode
 * finished in a pomcp_episodes_step take entries next, next + 1, ... in
 * ascending group order, a group that finds the queue empty is retired.  Every
 * one of a refilled group's trees is reset as pomcp_reset resets a tree (the RNG
 * stream counters carry on) and its records leave its search wave's shared log;
 * the group's kept merged record is zeroed and its one environment starts
 * under the new seed (the population's policy drawn per group).
 *
 * pomcp_episodes_group_queue_begin takes the group size itself: it neither
 * reads nor changes what pomcp_episodes_set_group stored (and
 * pomcp_episodes_queue_begin goes on refusing a stored group > 1).
 * POMCP_E_INVALID unless group >= 2 divides num_trees and n >= num_trees /
 * group; POMCP_E_UNSUPPORTED with pomcp_episodes_track_states(1) or
 * pomcp_episodes_track_belief_acc(1, ..) in force; every refusal comes before
 * any launch.  pomcp_episodes_begin and pomcp_reset end the mode.  While it is
 * active:
 *   - pomcp_episodes_step is the grouped step (num_sims per replica) followed
 *     by the queue's kernels; *live_out = unfinished + refilled groups;
 *   - pomcp_episodes_queue_rows has n rows, row.slot = the group;
 *     pomcp_episodes_queue_slots and _queue_finished have num_trees / group
 *     entries; pomcp_episodes_queue_timing is the queue's;
 *   - pomcp_episodes_results, _states, _pop_states and _merged_roots are the
 *     running episodes', one per group;
 *   - pomcp_episodes_queue_finished_merged: out[g] (host, [num_trees / group])
 *     = the kept pomcp_merged_root of the episode that ended in group g in the
 *     last pomcp_episodes_step, zeros where none ended.  POMCP_E_STATE without
 *     a running queue of groups. */
int pomcp_episodes_group_queue_begin(pomcp_ctx* ctx, int32_t group, const uint64_t* env_seeds,
                                     int32_t n, const double* pow_table, int32_t max_steps,
                                     int32_t until);
int pomcp_episodes_queue_finished_merged(pomcp_ctx* ctx, pomcp_merged_root* out);

/* Host twin of k_group_queue_trees' per-tree decision (csrc/episode_group_queue.h):
 * assign[g] = pomcp_host_queue_assign's decision for group g of num_groups
 * groups of `group` trees (num_groups * group = num_trees); masks_out[w] (one
 * per search wave of 64 trees) has bit l set when tree 64 w + l belongs to a
 * group that takes a new entry -- the mask k_log_drop gets.  Retiring (-1) and
 * playing (-2) groups contribute no bit. */
int pomcp_host_group_drop_masks(const int32_t* assign, int32_t num_groups, int32_t group,
                                int32_t num_trees, uint64_t* masks_out);

#ifdef __cplusplus
}
#endif

#endif /* POMCP_H_ */
