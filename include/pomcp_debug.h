/* pomcp_debug.h — diagnostics of libpomcp_hip.so (not part of the drop-in ABI). */
#ifndef POMCP_DEBUG_H_
#define POMCP_DEBUG_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* out[4*i + k] = {sqrt(a), a / b, a + 0.95 * b, (a - b) / (a + b)} computed on
 * device 0 in FP64 (checks the device FP64 path is correctly rounded). */
int pomcp_debug_fp_selftest(const double* a, const double* b, int32_t n, double* out);
/* out[2i] = rcp_nr(x[i]), out[2i + 1] = rsq_nr(x[i]) on device 0: the FP64
 * 1/x and 1/sqrt(x) of k_search's fast UCB scores (hardware estimate + two
 * Newton steps), whose error bound decides when the exact scores are needed. */
int pomcp_debug_fast_recip(const double* x, int32_t n, double* out);
/* out[i] = host_exp(x[i]) on device 0 (FP64): the I-NTMCP softmax's exp, a
 * bit-exact restatement of the host libm's exp (csrc/host_exp.h). */
int pomcp_debug_exp(const double* x, int32_t n, double* out);
/* The same function evaluated on the host CPU (no GPU needed). */
int pomcp_debug_host_exp(const double* x, int32_t n, double* out);
/* k_search phase cycles per wave, [waves][16] (libpomcp_hip built with
 * -DPOMCP_PHASE_TIMING; POMCP_E_UNSUPPORTED otherwise).  The first call
 * enables collection (count = 0); later calls copy the last search's values
 * when capacity >= count. */
typedef struct pomcp_ctx pomcp_ctx;
int pomcp_debug_phase_timing(pomcp_ctx* ctx, uint64_t* out, int32_t capacity, int32_t* count);
/* k_im_search phase cycles per wave (libpomcp_hip built with
 * -DPOMCP_PHASE_TIMING; POMCP_E_UNSUPPORTED otherwise), same protocol as
 * pomcp_debug_phase_timing (tools/phase_timing_im.py). */
typedef struct intmcp_ctx intmcp_ctx;
int intmcp_debug_phase_timing(intmcp_ctx* ctx, uint64_t* out, int32_t capacity, int32_t* count);
/* k_search_lds (the wave-per-tree kernel): polls of a late step-tree hand-off
 * before the search wave stops its producer waves and computes the rest of the
 * launch itself (0 = the default, ~0.1 s); results are the same either way. */
int pomcp_debug_set_spin_limit(pomcp_ctx* ctx, int32_t polls);
/* I-NTMCP: the other agent's softmax (sample_action, intmcp.py:763-791) takes
 * its choice from bounded FP32 weights and falls back to the exact FP64 path
 * near a cumulative weight; `slack` (>= 1, default 1) widens that bound, so a
 * large value sends most draws down the exact path (results stay exact).  From
 * this call on the exact-path draws are counted: intmcp_debug_exact_draws. */
int intmcp_debug_set_softmax_slack(intmcp_ctx* ctx, float slack);
int intmcp_debug_exact_draws(intmcp_ctx* ctx, uint64_t* count);
/* I-NTMCP: what one tree's arenas of one pair hold, over their whole capacity
 * (tests of intmcp_reset_pairs; slow): out[0] = the node blocks in [0,
 * max_nodes) with any non-zero byte (line or action records), out[1] = one past
 * the highest such block (0: none), out[2] = the obs-child map slots that are
 * not the empty entry. */
int intmcp_debug_arena_scan(intmcp_ctx* ctx, int32_t pair, int32_t tree, int64_t out[3]);
/* I-NTMCP episode queue: the bytes the arena clear (k_im_clear_pairs) stored
 * since intmcp_episodes_queue_begin -- node blocks and obs-child maps of every
 * refilled slot (tools/batched_episodes_timing.py --intmcp-queue). */
int intmcp_debug_queue_cleared_bytes(intmcp_ctx* ctx, int64_t* bytes);
/* k_search's fast UCB / PUCB selection (DESIGN.md §4 "Fast selection") takes
 * the fast scores' leader unless an action with different statistics scores
 * within `rel` of it relative to their magnitudes, and then decides with the
 * exact FP64 scores (mcts.py:502-546).  rel >= 1e-12 (the default, above the
 * fast scores' proven error) keeps results exact; a large rel (e.g. 1e-4)
 * sends most selections down the exact path.  pomcp_root_stats.n_exact_selects
 * counts them per tree and search. */
int pomcp_debug_set_select_margin(pomcp_ctx* ctx, double rel);
/* Only the first n (1..6) inline obs-child slots of each action node are used,
 * the overflow map holds the rest (tests of that path).  Before the first search. */
int pomcp_debug_set_inline_slots(pomcp_ctx* ctx, int32_t n);
/* The obs-child overflow map's generation (the 14-bit tag in bits 50..63 of a
 * map key; it advances on every reset, restore, re-root and queue refill and
 * the map is cleared when it wraps): tree b's becomes gen[b], [num_trees]
 * values in 1..16383 (POMCP_E_INVALID otherwise).  Synchronises the context's
 * stream first.  The map itself is not touched: entries already stored under
 * gen[b] become live again, so a test chooses values no stored entry carries. */
int pomcp_debug_set_map_generation(pomcp_ctx* ctx, const int32_t* gen);
/* One tree's overflow map, counted over its whole capacity: out[0] = the slots
 * whose generation is the tree's current one (live), out[1] = the slots of any
 * other non-zero generation (stale), out[2] = the tree's current generation. */
int pomcp_debug_map_scan(pomcp_ctx* ctx, int32_t tree, int64_t out[3]);
/* Device time of k_belief_stats alone (pomcp_belief_stats without its copies):
 * after one untimed launch, `reps` launches between two events on the context
 * stream; *ms_per_launch = elapsed / reps.  states as pomcp_belief_stats. */
int pomcp_debug_belief_stats_ms(pomcp_ctx* ctx, const uint32_t* states, int32_t reps,
                                float* ms_per_launch);
/* The compile-time depth limit of the tree-per-lane kernel (k_search) that the
 * context's next search launch would use: its depth_limit when that is 1..3
 * and the search is not type-based, else 0 = the generic kernel with a runtime
 * limit (also when POMCP_SEARCH_DEPTH_SPEC=0 is set in the environment, or the
 * launch goes to the wave-per-tree kernel).  Results are the same either way. */
int pomcp_debug_search_depth_spec(const pomcp_ctx* ctx);
/* One search wave's shared particle log (trees 64 wave .. 64 wave + 63) in
 * record order: *count = its records, of which the first min(count, capacity)
 * go to ids / v0 / v1 (and aux, on a type-based context; NULL: not wanted).
 * A record's tree lane is ids[i] >> 26. */
int pomcp_debug_get_wave_log(pomcp_ctx* ctx, int32_t wave, uint32_t* ids, uint32_t* v0, uint32_t* v1,
                             uint32_t* aux, int32_t capacity, int32_t* count);
/* Launches k_log_drop with the caller's masks (one uint64 per search wave: bit
 * l = drop the records of tree lane l).  The trees' own log counts are not
 * touched: a test of the kernel, not a way to reset a tree. */
int pomcp_debug_log_drop(pomcp_ctx* ctx, const uint64_t* masks);
/* The context's environment step and observation key on the device, through
 * the device functions the search kernels call, one case per lane: for case i,
 * in[5i..5i+4] = {state[0], state[1], the ego's action, the other agent's
 * action, the execution-order draw j (Driving: 0 = agent 1 moves first;
 * PursuitEvasion: ignored)} and out[8i..8i+7] = {next[0], next[1], the ego's
 * reward's low and high words, its done flag, its observation key's low and
 * high words, 0}.  The ego is the context's.  States must be ones the model
 * produces (a Driving vehicle's min-distance field at most its cell's distance). */
int pomcp_debug_env_step(pomcp_ctx* ctx, const uint32_t* in, int32_t n, uint32_t* out);
/* Host: pomcp_pp_step (pomcp.h) with the draw given (j < 2^25) instead of taken
 * from a stream, and what the step did, for the tests' conditions: rules_out[k]
 * the rule that decided prey k's move (0 a predator, 1 another prey, 2 neither;
 * -1 not live), blocked_out[i] whether predator i's move was held in place.
 * Either may be NULL. */
int pomcp_debug_pp_step_draw(const pomcp_pp_grid* g, const uint32_t state[2],
                             const int32_t actions[2], uint32_t j, uint32_t next_out[2],
                             double rewards_out[2], int32_t terminated_out[2],
                             uint64_t obs_keys_out[2], int32_t rules_out[3],
                             int32_t blocked_out[2]);
#ifdef __cplusplus
}
#endif
#endif
