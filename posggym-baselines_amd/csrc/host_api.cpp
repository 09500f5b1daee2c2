// Host-only entry points of libpomcp_hip.so (include/pomcp.h, pomcp_debug.h):
// the environment side of the episode loop (Driving-v1 / PursuitEvasion-v1 /
// CooperativeReaching-v0 from the same driving.h / pursuit_evasion.h /
// cooperative_reaching.h the kernels use), the host RNG
// words and the host log / exp tables -- the reference's step / obs / RNG
// contract (mcts.py:181-198, 333, 418; exp_utils.py:481).
//
// Plain C++ with no HIP dependency: pomcp_capi.hip includes it into the
// product library, and tests/test_host_sanitize.py compiles it on its own
// with -fsanitize=address,undefined into an executable that serves the same
// calls (tests/native/host_rpc.cpp), so the host code runs under the
// sanitizers through the same Python tests.
#if !defined(__HIPCC__) && !defined(__HIP__)
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif
#include <stdint.h>

#include <climits>
#include <cmath>
#include <cstring>

#include "belief_stats.h"
#include "cooperative_reaching.h"
#include "driving.h"
#include "driving_policy.h"
#include "episode_group.h"
#include "episode_group_queue.h"
#include "episode_queue.h"
#include "episode_step.h"
#include "host_exp.h"
#include "intmcp_episode.h"
#include "philox.h"
#include "predator_prey.h"
#include "pursuit_evasion.h"
#include "tm_prior.h"
#include "../../include/pomcp.h"
#include "../../include/pomcp_debug.h"

using namespace pb;

namespace {
// (the tables of the calling thread's last grid are kept: a host episode loop or
// a test steps one grid many times, and building them is most of a step's cost)
void make_model(const pomcp_grid* g, DrvModel* m) {
  static_assert(sizeof(pomcp_grid) == sizeof(DrvGrid), "pomcp_grid is DrvGrid's layout");
  thread_local DrvModel last;
  thread_local bool have = false;
  if (!have || std::memcmp(&last.g, g, sizeof(DrvGrid)) != 0) {
    have = false;
    std::memcpy(&last.g, g, sizeof(DrvGrid));
    build_model_tables(last.g, &last);
    have = true;
  }
  *m = last;
}

// f(E{}, model) with the episode environment E of env_id (episode_step.h) and
// its tables built from `grid`
template <class F>
void with_host_env(int32_t env_id, const void* grid, F&& f) {
  if (env_id == POMCP_ENV_DRIVING) {
    DrvModel m;
    make_model(reinterpret_cast<const pomcp_grid*>(grid), &m);
    f(EpDriving{}, m);
  } else if (env_id == POMCP_ENV_PURSUIT_EVASION) {
    PeModel m;
    build_pe_model(*reinterpret_cast<const pomcp_pe_grid*>(grid), &m);
    f(EpPursuitEvasion{}, m);
  } else if (env_id == POMCP_ENV_PREDATOR_PREY) {
    PpModel m;
    build_pp_model(*reinterpret_cast<const pomcp_pp_grid*>(grid), &m);
    f(EpPredatorPrey{}, m);
  } else {
    CrModel m;
    build_cr_model(*reinterpret_cast<const pomcp_cr_grid*>(grid), &m);
    f(EpCoopReaching{}, m);
  }
}

int host_env_actions(int32_t env_id) { return env_id == POMCP_ENV_PURSUIT_EVASION ? 4 : 5; }
}  // namespace

extern "C" {

// ---------------------------------------------------------------- host model

int pomcp_driving_sample_initial_state(const pomcp_grid* g, uint64_t seed, uint32_t tree,
                                       uint32_t* model_ctr, uint32_t state_out[2]) {
  if (!g || !model_ctr || !state_out) return POMCP_E_INVALID;
  const DrvGrid& gg = *reinterpret_cast<const DrvGrid*>(g);
  Streams s;
  s.seed = seed;
  s.tree = tree;
  for (int k = 0; k < 5; ++k) s.ctr[k] = 0;
  s.ctr[2] = *model_ctr;
  drv_sample_initial_state2(gg, [&](uint32_t n) { return s.model(n); }, &state_out[0],
                            &state_out[1]);
  *model_ctr = s.ctr[2];
  return POMCP_OK;
}

int pomcp_driving_step(const pomcp_grid* g, uint64_t seed, uint32_t tree, uint32_t* model_ctr,
                       const uint32_t state[2], const int32_t actions[2], uint32_t next_out[2],
                       double rewards_out[2], int32_t terminated_out[2],
                       uint64_t obs_keys_out[2]) {
  if (!g || !model_ctr || !state || !actions || !next_out) return POMCP_E_INVALID;
  DrvModel m;
  make_model(g, &m);
  Streams s;
  s.seed = seed;
  s.tree = tree;
  for (int k = 0; k < 5; ++k) s.ctr[k] = 0;
  s.ctr[2] = *model_ctr;
  const uint32_t j = s.model(2);   // execution-order shuffle
  *model_ctr = s.ctr[2];
  drv_step2_fast(m, state[0], state[1], actions[0], actions[1], j, &next_out[0], &next_out[1]);
  for (int i = 0; i < 2; ++i) {
    if (rewards_out) rewards_out[i] = drv_reward_fast(m, state[i], next_out[i]);
    if (terminated_out) terminated_out[i] = veh_done(next_out[i]) ? 1 : 0;
  }
  if (obs_keys_out) {
    obs_keys_out[0] = obs_key_fast(m, next_out[0], next_out[1]);
    obs_keys_out[1] = obs_key_fast(m, next_out[1], next_out[0]);
  }
  return POMCP_OK;
}

int pomcp_driving_obs(const pomcp_grid* g, const uint32_t state[2], uint64_t obs_keys_out[2]) {
  if (!g || !state || !obs_keys_out) return POMCP_E_INVALID;
  DrvModel m;
  make_model(g, &m);
  obs_keys_out[0] = obs_key_fast(m, state[0], state[1]);
  obs_keys_out[1] = obs_key_fast(m, state[1], state[0]);
  return POMCP_OK;
}

// The shortest-path agents' rule (driving_policy.h), the code the kernels run.
int pomcp_host_driving_policy_actions(const pomcp_grid* g, int64_t n, const uint32_t* own,
                                      const uint32_t* other, int32_t caution, int32_t vmax,
                                      int32_t* out) {
  if (!g || n < 0 || (n > 0 && (!own || !other || !out)) ||
      !drv_policy_kind_ok(POMCP_POLICY_DRIVING_SHORTEST_PATH, caution, vmax))
    return POMCP_E_INVALID;
  const DrvGrid& gg = *reinterpret_cast<const DrvGrid*>(g);
  for (int64_t i = 0; i < n; ++i) out[i] = drv_sp_action(gg, own[i], other[i], caution, vmax);
  return POMCP_OK;
}

// ------------------------------------------------- host CooperativeReaching

int pomcp_cr_sample_initial_state(const pomcp_cr_grid* g, uint64_t seed, uint32_t tree,
                                  uint32_t* model_ctr, uint32_t state_out[2]) {
  if (!g || !model_ctr || !state_out || !cr_grid_ok(*g)) return POMCP_E_INVALID;
  CrModel m;
  build_cr_model(*g, &m);
  Streams s;
  s.seed = seed;
  s.tree = tree;
  for (int k = 0; k < 5; ++k) s.ctr[k] = 0;
  s.ctr[2] = *model_ctr;
  cr_sample_initial_state(m, [&](uint32_t n) { return s.model(n); }, &state_out[0], &state_out[1]);
  *model_ctr = s.ctr[2];
  return POMCP_OK;
}

int pomcp_cr_sample_agent_initial_state(const pomcp_cr_grid* g, int32_t agent, uint64_t obs_key,
                                        uint64_t seed, uint32_t tree, uint32_t* model_ctr,
                                        uint32_t state_out[2]) {
  if (!g || !model_ctr || !state_out || (agent != 0 && agent != 1) || !cr_grid_ok(*g))
    return POMCP_E_INVALID;
  CrModel m;
  build_cr_model(*g, &m);
  Streams s;
  s.seed = seed;
  s.tree = tree;
  for (int k = 0; k < 5; ++k) s.ctr[k] = 0;
  s.ctr[2] = *model_ctr;
  const bool ok = cr_sample_agent_initial(m, agent, obs_key, [&](uint32_t n) { return s.model(n); },
                                          &state_out[0], &state_out[1]);
  *model_ctr = s.ctr[2];
  return ok ? POMCP_OK : POMCP_E_INVALID;
}

// false: a word whose cell lies outside the grid
static bool cr_state_ok(const CrModel& m, const uint32_t state[2]) {
  for (int i = 0; i < 2; ++i)
    if ((int)cr_x(state[i]) >= m.size || (int)cr_y(state[i]) >= m.size) return false;
  return true;
}

int pomcp_cr_step(const pomcp_cr_grid* g, const uint32_t state[2], const int32_t actions[2],
                  uint32_t next_out[2], double rewards_out[2], int32_t terminated_out[2],
                  uint64_t obs_keys_out[2]) {
  if (!g || !state || !actions || !next_out || !rewards_out || !terminated_out || !obs_keys_out ||
      !cr_grid_ok(*g))
    return POMCP_E_INVALID;
  for (int i = 0; i < 2; ++i)
    if (actions[i] < 0 || actions[i] > 4) return POMCP_E_INVALID;
  CrModel m;
  build_cr_model(*g, &m);
  if (!cr_state_ok(m, state)) return POMCP_E_INVALID;
  double r;
  cr_step(m, state[0], state[1], (uint32_t)actions[0], (uint32_t)actions[1], &next_out[0],
          &next_out[1], &r);
  for (int i = 0; i < 2; ++i) {
    rewards_out[i] = r;
    terminated_out[i] = cr_done(next_out[0], next_out[1]) ? 1 : 0;
    obs_keys_out[i] = cr_obs_key(m, i, next_out[0], next_out[1]);
  }
  return POMCP_OK;
}

int pomcp_cr_obs(const pomcp_cr_grid* g, const uint32_t state[2], uint64_t obs_keys_out[2]) {
  if (!g || !state || !obs_keys_out || !cr_grid_ok(*g)) return POMCP_E_INVALID;
  CrModel m;
  build_cr_model(*g, &m);
  if (!cr_state_ok(m, state)) return POMCP_E_INVALID;
  for (int i = 0; i < 2; ++i) obs_keys_out[i] = cr_obs_key(m, i, state[0], state[1]);
  return POMCP_OK;
}

// The heuristic agents' rule (cooperative_reaching.h), the code the kernels run.
int pomcp_host_cr_policy_actions(const pomcp_cr_grid* g, int64_t n, const uint32_t* own,
                                 int32_t rule, int32_t* out) {
  if (!g || n < 0 || (n > 0 && (!own || !out)) || !cr_grid_ok(*g) ||
      !cr_policy_kind_ok(POMCP_POLICY_CR_GOAL, rule, 0))
    return POMCP_E_INVALID;
  CrModel m;
  build_cr_model(*g, &m);
  for (int64_t i = 0; i < n; ++i) out[i] = cr_goal_action(m, own[i], rule);
  return POMCP_OK;
}

// The prior line of a node under reactive ego policies (tm_prior.h), the code
// k_search runs: out[i][0 .. 5) for the ego word own[i].
int pomcp_host_cr_prior_lines(const pomcp_cr_grid* g, int32_t num_ego, const double* ego_pi,
                              const double* expected_prior, const pomcp_policy_kinds* kinds,
                              const double* expected_meta, int32_t code, int64_t n,
                              const uint32_t* own, double* out) {
  constexpr int A = 5;
  if (!g || !ego_pi || !expected_prior || !kinds || !expected_meta || n < 0 ||
      (n > 0 && (!own || !out)) || !cr_grid_ok(*g) || num_ego < 1 || num_ego > kTmEgoMax ||
      code < 0 || code > num_ego)
    return POMCP_E_INVALID;
  double prior[kTmEgoMax + 1][kTmEgoMax] = {};
  TmEgo e{};
  for (int a = 0; a < A; ++a) prior[0][a] = expected_prior[a];
  for (int k = 0; k < num_ego; ++k) {
    for (int a = 0; a < A; ++a) prior[k + 1][a] = ego_pi[k * POMCP_MAX_ACTIONS + a];
    if (kinds->kind[k] == POMCP_POLICY_FIXED) continue;
    if (!cr_policy_kind_ok(kinds->kind[k], kinds->param0[k], kinds->param1[k]))
      return POMCP_E_INVALID;
    e.any = 1;
    e.kind[k] = kinds->kind[k];
    e.p0[k] = kinds->param0[k];
    e.p1[k] = kinds->param1[k];
  }
  for (int k = 0; k < num_ego; ++k) e.w[k] = expected_meta[k];
  CrModel m;
  build_cr_model(*g, &m);
  for (int64_t i = 0; i < n; ++i) {
    const uint32_t v = own[i];
    tm_prior_line(prior, e, num_ego, A, code,
                  [&](int k) { return cr_goal_action(m, v, e.p0[k]); }, out + i * A);
  }
  return POMCP_OK;
}

// ------------------------------------------------------- host PredatorPrey

namespace {
Streams pp_streams(uint64_t seed, uint32_t tree, uint32_t model_ctr) {
  Streams s;
  s.seed = seed;
  s.tree = tree;
  for (int k = 0; k < 5; ++k) s.ctr[k] = 0;
  s.ctr[2] = model_ctr;
  return s;
}
}  // namespace

int pomcp_pp_sample_initial_state(const pomcp_pp_grid* g, uint64_t seed, uint32_t tree,
                                  uint32_t* model_ctr, uint32_t state_out[2]) {
  if (!g || !model_ctr || !state_out || !pp_grid_ok(*g)) return POMCP_E_INVALID;
  PpModel m;
  build_pp_model(*g, &m);
  Streams s = pp_streams(seed, tree, *model_ctr);
  pp_sample_initial_state(m, [&](uint32_t n) { return s.model(n); }, &state_out[0], &state_out[1]);
  *model_ctr = s.ctr[2];
  return POMCP_OK;
}

int pomcp_pp_sample_agent_initial_state(const pomcp_pp_grid* g, int32_t agent, uint64_t obs_key,
                                        uint64_t seed, uint32_t tree, uint32_t* model_ctr,
                                        uint32_t state_out[2]) {
  if (!g || !model_ctr || !state_out || (agent != 0 && agent != 1) || !pp_grid_ok(*g))
    return POMCP_E_INVALID;
  PpModel m;
  build_pp_model(*g, &m);
  Streams s = pp_streams(seed, tree, *model_ctr);
  const bool ok = pp_sample_agent_initial(m, agent, obs_key, [&](uint32_t n) { return s.model(n); },
                                          &state_out[0], &state_out[1]);
  *model_ctr = s.ctr[2];
  return ok ? POMCP_OK : POMCP_E_INVALID;
}

// (pomcp_debug.h: the step with the draw given, and what it did)
int pomcp_debug_pp_step_draw(const pomcp_pp_grid* g, const uint32_t state[2],
                             const int32_t actions[2], uint32_t j, uint32_t next_out[2],
                             double rewards_out[2], int32_t terminated_out[2],
                             uint64_t obs_keys_out[2], int32_t rules_out[3],
                             int32_t blocked_out[2]) {
  if (!g || !state || !actions || !next_out || !rewards_out || !terminated_out || !obs_keys_out ||
      !pp_grid_ok(*g) || j >= kPpStepRange)
    return POMCP_E_INVALID;
  for (int i = 0; i < 2; ++i)
    if (actions[i] < 0 || actions[i] > 4) return POMCP_E_INVALID;
  PpModel m;
  build_pp_model(*g, &m);
  if (!pp_state_ok(m, state)) return POMCP_E_INVALID;
  uint32_t n;
  PpStepInfo info;
  pp_step_info(m, state[0], state[1], (uint32_t)actions[0], (uint32_t)actions[1], j, &next_out[0],
               &next_out[1], &n, &info);
  for (int i = 0; i < 2; ++i) {
    rewards_out[i] = (double)n * m.reward;
    terminated_out[i] = pp_done(next_out[0]) ? 1 : 0;
    obs_keys_out[i] = pp_obs_key(m, i, next_out[0], next_out[1]);
    if (blocked_out) blocked_out[i] = info.blocked[i];
  }
  for (int k = 0; rules_out && k < kPpMaxPrey; ++k) rules_out[k] = info.rule[k];
  return POMCP_OK;
}

int pomcp_pp_step(const pomcp_pp_grid* g, const uint32_t state[2], const int32_t actions[2],
                  uint64_t seed, uint32_t tree, uint32_t* model_ctr, uint32_t next_out[2],
                  double rewards_out[2], int32_t terminated_out[2], uint64_t obs_keys_out[2]) {
  if (!model_ctr) return POMCP_E_INVALID;
  Streams s = pp_streams(seed, tree, *model_ctr);
  const uint32_t j = s.model(kPpStepRange);
  const int rc = pomcp_debug_pp_step_draw(g, state, actions, j, next_out, rewards_out,
                                          terminated_out, obs_keys_out, nullptr, nullptr);
  if (rc == POMCP_OK) *model_ctr = s.ctr[2];
  return rc;
}

int pomcp_pp_obs(const pomcp_pp_grid* g, const uint32_t state[2], uint64_t obs_keys_out[2]) {
  if (!g || !state || !obs_keys_out || !pp_grid_ok(*g)) return POMCP_E_INVALID;
  PpModel m;
  build_pp_model(*g, &m);
  if (!pp_state_ok(m, state)) return POMCP_E_INVALID;
  for (int i = 0; i < 2; ++i) obs_keys_out[i] = pp_obs_key(m, i, state[0], state[1]);
  return POMCP_OK;
}

// The heuristic agents' rule (predator_prey_policy.h), the code the kernels run.
int pomcp_host_pp_policy_pi(const pomcp_pp_grid* g, int64_t n, const uint32_t* w0,
                            const uint32_t* w1, int32_t agent, int32_t rule, double* out) {
  if (!g || n < 0 || (n > 0 && (!w0 || !w1 || !out)) || (agent != 0 && agent != 1) ||
      !pp_grid_ok(*g) || !pp_policy_kind_ok(POMCP_POLICY_PP_HEURISTIC, rule, 0))
    return POMCP_E_INVALID;
  PpModel m;
  build_pp_model(*g, &m);
  for (int64_t i = 0; i < n; ++i) pp_heuristic_pi(m, agent, w0[i], w1[i], rule, out + i * 5);
  return POMCP_OK;
}

int pomcp_host_pp_policy_actions(const pomcp_pp_grid* g, int64_t n, const uint32_t* w0,
                                 const uint32_t* w1, int32_t agent, int32_t rule,
                                 const uint32_t* words, int32_t* out) {
  if (!g || n < 0 || (n > 0 && (!w0 || !w1 || !words || !out)) || (agent != 0 && agent != 1) ||
      !pp_grid_ok(*g) || !pp_policy_kind_ok(POMCP_POLICY_PP_HEURISTIC, rule, 0))
    return POMCP_E_INVALID;
  PpModel m;
  build_pp_model(*g, &m);
  for (int64_t i = 0; i < n; ++i)
    out[i] = pp_heuristic_action(m, agent, w0[i], w1[i], rule, words[i]);
  return POMCP_OK;
}

// ---------------------------------------------------------- host RNG streams

int pomcp_philox_words(uint64_t seed, uint32_t tree, uint32_t stream, uint32_t first, int32_t n,
                       uint32_t* out) {
  if (n < 0 || (n > 0 && !out)) return POMCP_E_INVALID;
  for (int32_t k = 0; k < n; ++k) out[k] = philox_word(seed, tree, stream, first + (uint32_t)k);
  return POMCP_OK;
}

// ---------------------------------------------------------- host log(N) table

// out[i] = log((double)i) for i in [first, first + n), out[0] of i = 0 is 0.0:
// the host C library's log, the function Python's math.log calls for a float
// (Modules/mathmodule.c), so the table is math.log's bit for bit at C speed
// (tests/test_host_exp.py checks it against math.log).
int pomcp_host_log_table(int64_t first, int64_t n, double* out) {
  if (first < 0 || n < 0 || (n > 0 && !out)) return POMCP_E_INVALID;
  for (int64_t k = 0; k < n; ++k) {
    const int64_t i = first + k;
    out[k] = i == 0 ? 0.0 : std::log((double)i);
  }
  return POMCP_OK;
}

// ---------------------------------------------------- host belief statistics

// The counts k_belief_stats (belief_stats.hip) makes of one tree's root belief,
// record by record with the same bel_classify (utils.py:292-339).
int pomcp_host_belief_counts(const uint32_t* records4, int64_t n, const uint32_t* state,
                             int32_t num_other, pomcp_belief_counts* out) {
  if (!out || n < 0 || n > INT_MAX || (n > 0 && !records4) || num_other < 0 ||
      num_other > POMCP_MAX_TYPE_POLICIES)
    return POMCP_E_INVALID;
  pomcp_belief_counts c;
  std::memset(&c, 0, sizeof(c));
  c.belief_size = (int32_t)n;
  const int has_q = state != nullptr;
  const uint32_t q0 = has_q ? state[0] : 0u, q1 = has_q ? state[1] : 0u;
  for (int64_t i = 0; i < n; ++i) {
    const uint32_t* r = records4 + 4 * i;
    // (a plain belief's aux word is not read)
    const uint32_t k = bel_classify(r[1], r[2], num_other ? r[3] : 0u, q0, q1, has_q,
                                    (uint32_t)num_other);
    c.state_matches += (k & kBelMatch) ? 1 : 0;
    if (k & kBelBadAux)
      c.error = POMCP_E_INVALID;
    else if (num_other)
      c.policy_hist[k >> kBelPolShift] += 1;
  }
  if (!has_q) c.state_matches = -1;
  *out = c;
  return c.error;
}

// ---------------------------------------------------------- host PursuitEvasion

int pomcp_pe_sample_initial_state(const pomcp_pe_grid* g, uint64_t seed, uint32_t tree,
                                  uint32_t* model_ctr, uint32_t state_out[2]) {
  if (!g || !model_ctr || !state_out) return POMCP_E_INVALID;
  PeModel m;
  build_pe_model(*g, &m);
  Streams s;
  s.seed = seed;
  s.tree = tree;
  for (int k = 0; k < 5; ++k) s.ctr[k] = 0;
  s.ctr[2] = *model_ctr;
  pe_sample_initial_state(m, [&](uint32_t n) { return s.model(n); }, &state_out[0], &state_out[1]);
  *model_ctr = s.ctr[2];
  return POMCP_OK;
}

int pomcp_pe_step(const pomcp_pe_grid* g, const uint32_t state[2], const int32_t actions[2],
                  uint32_t next_out[2], double rewards_out[2], int32_t terminated_out[2],
                  uint64_t obs_keys_out[2]) {
  if (!g || !state || !actions || !next_out || !rewards_out || !terminated_out || !obs_keys_out)
    return POMCP_E_INVALID;
  for (int i = 0; i < 2; ++i)
    if (actions[i] < 0 || actions[i] > 3) return POMCP_E_INVALID;
  PeModel m;
  build_pe_model(*g, &m);
  uint32_t prog, outcome;
  pe_step(m, state[0], state[1], (uint32_t)actions[0], (uint32_t)actions[1], &next_out[0],
          &next_out[1], &prog, &outcome);
  for (int i = 0; i < 2; ++i) {
    rewards_out[i] = pe_reward(m, i, state[0], prog, outcome);
    terminated_out[i] = pe_done(next_out[0]) ? 1 : 0;
    obs_keys_out[i] = pe_obs_key(m, i, next_out[0], next_out[1]);
  }
  return POMCP_OK;
}

int pomcp_pe_obs(const pomcp_pe_grid* g, const uint32_t state[2], uint64_t obs_keys_out[2]) {
  if (!g || !state || !obs_keys_out) return POMCP_E_INVALID;
  PeModel m;
  build_pe_model(*g, &m);
  for (int i = 0; i < 2; ++i) obs_keys_out[i] = pe_obs_key(m, i, state[0], state[1]);
  return POMCP_OK;
}

// ------------------------------------------------------- host episode step

// The per-tree work of k_episode_reset / k_episode_step (pomcp_episode.hip) on
// the host, through the same episode_step.h.
namespace {
bool episode_env_ok(int32_t env_id, const void* grid, int32_t ego) {
  if (grid == nullptr || (ego != 0 && ego != 1)) return false;
  if (env_id == POMCP_ENV_COOPERATIVE_REACHING)
    return cr_grid_ok(*reinterpret_cast<const pomcp_cr_grid*>(grid));
  if (env_id == POMCP_ENV_PREDATOR_PREY)
    return pp_grid_ok(*reinterpret_cast<const pomcp_pp_grid*>(grid));
  return env_id == POMCP_ENV_DRIVING || env_id == POMCP_ENV_PURSUIT_EVASION;
}

}  // namespace

int pomcp_host_episode_reset(int32_t env_id, const void* grid, int32_t ego, uint64_t env_seed,
                             pomcp_episode_state* st, uint64_t* obs_key_out) {
  if (!episode_env_ok(env_id, grid, ego) || !st || !obs_key_out) return POMCP_E_INVALID;
  with_host_env(env_id, grid, [&](auto e, const auto& m) {
    *obs_key_out = episode_reset<decltype(e)>(m, ego, env_seed, st);
  });
  return POMCP_OK;
}

int pomcp_host_episode_step(int32_t env_id, const void* grid, int32_t ego,
                            const pomcp_episode_step_in* in, const double* pow_table,
                            int32_t max_steps, int32_t until, pomcp_episode_state* st,
                            pomcp_episode_step_out* out) {
  if (!episode_env_ok(env_id, grid, ego) || !in || !pow_table || !st || !out || max_steps < 1 ||
      (until != POMCP_UNTIL_AGENT_DONE && until != POMCP_UNTIL_ALL_DONE))
    return POMCP_E_INVALID;
  with_host_env(env_id, grid, [&](auto e, const auto& m) {
    episode_step<decltype(e)>(m, ego, *in, pow_table, max_steps, until, st, out);
  });
  return POMCP_OK;
}

// The population overloads of episode_step.h (k_episode_reset / k_episode_step
// with a population set); a null pop is the two entry points above.
int pomcp_host_episode_reset_pop(int32_t env_id, const void* grid, int32_t ego, uint64_t env_seed,
                                 const pomcp_episode_population* pop, pomcp_episode_state* st,
                                 pomcp_episode_pop_state* ps, uint64_t* obs_key_out) {
  if (!episode_env_ok(env_id, grid, ego) || !st || !obs_key_out) return POMCP_E_INVALID;
  pomcp_episode_pop_state local;
  if (!ps) {
    if (pop) return POMCP_E_INVALID;
    ps = &local;
  }
  EpPopTables t;
  if (pop && !ep_pop_tables(*pop, host_env_actions(env_id), &t))
    return POMCP_E_INVALID;
  const EpPopTables* tp = pop ? &t : nullptr;
  with_host_env(env_id, grid, [&](auto e, const auto& m) {
    *obs_key_out = episode_reset<decltype(e)>(m, ego, env_seed, tp, st, ps);
  });
  return POMCP_OK;
}

// (kinds: the population's pomcp_policy_kinds, null for all fixed)
int pomcp_host_episode_step_pop_kinds(int32_t env_id, const void* grid, int32_t ego,
                                      const pomcp_episode_step_in* in, const double* pow_table,
                                      int32_t max_steps, int32_t until,
                                      const pomcp_episode_population* pop,
                                      const pomcp_policy_kinds* kinds,
                                      const pomcp_episode_pop_state* ps, pomcp_episode_state* st,
                                      pomcp_episode_step_out* out) {
  if (!episode_env_ok(env_id, grid, ego) || !in || !pow_table || !st || !out || max_steps < 1 ||
      (until != POMCP_UNTIL_AGENT_DONE && until != POMCP_UNTIL_ALL_DONE) || (kinds && !pop))
    return POMCP_E_INVALID;
  EpPopTables t;
  if (pop) {
    if (!ps || !ep_pop_tables(*pop, host_env_actions(env_id), &t) ||
        ps->policy_index < 0 || ps->policy_index >= t.n)
      return POMCP_E_INVALID;
    int rc = POMCP_OK;
    with_host_env(env_id, grid, [&](auto e, const auto&) { rc = ep_pop_kinds<decltype(e)>(kinds, &t); });
    if (rc != POMCP_OK) return rc;
  }
  const EpPopTables* tp = pop ? &t : nullptr;
  const int k = pop ? ps->policy_index : -1;
  with_host_env(env_id, grid, [&](auto e, const auto& m) {
    episode_step<decltype(e)>(m, ego, *in, pow_table, max_steps, until, tp, k, st, out);
  });
  return POMCP_OK;
}

int pomcp_host_episode_step_pop(int32_t env_id, const void* grid, int32_t ego,
                                const pomcp_episode_step_in* in, const double* pow_table,
                                int32_t max_steps, int32_t until,
                                const pomcp_episode_population* pop,
                                const pomcp_episode_pop_state* ps, pomcp_episode_state* st,
                                pomcp_episode_step_out* out) {
  return pomcp_host_episode_step_pop_kinds(env_id, grid, ego, in, pow_table, max_steps, until, pop,
                                           nullptr, ps, st, out);
}

// The per-group decision of k_group_episode_step (pomcp_episode_group.hip) on
// the host, through the same episode_group.h: the replicas' flags in chunks of
// kEpGroupChunk, each chunk summarised in replica order (the kernel's ballots),
// the chunks folded in order; then the planner's part of the episode step.
int pomcp_host_episode_group_step_in(const int32_t* flags, int32_t group, int32_t num_sims,
                                     const pomcp_merged_root* merged,
                                     pomcp_episode_step_in* in_out, int32_t* keep_out) {
  if (!flags || !merged || !in_out || group < 1 || num_sims < 0 ||
      (int64_t)group * num_sims > INT32_MAX)
    return POMCP_E_INVALID;
  EpGroupFlags f = ep_group_none();
  for (int32_t k0 = 0; k0 < group; k0 += kEpGroupChunk) {
    EpGroupFlags c = ep_group_none();
    for (int32_t k = k0; k < group && k < k0 + kEpGroupChunk; ++k) {
      const int32_t* r = flags + 3 * (int64_t)k;
      if (r[0] == 0) c.any_live = 1;
      if (c.update_error == 0) c.update_error = r[1];
      if (c.search_error == 0) c.search_error = r[2];
    }
    ep_group_fold(&f, c);
  }
  ep_group_step_in(f, *merged, group, num_sims, in_out);
  // (for a planner whose root was not absorbing before the step)
  if (keep_out) *keep_out = ep_group_real(0, *in_out) ? 1 : 0;
  return POMCP_OK;
}

// The per-pair work of k_im_episode_step / k_im_episode_unpark
// (intmcp_episode.hip) on the host, through the same intmcp_episode.h.
int intmcp_host_episode_step(int32_t env_id, const void* grid, int32_t ego,
                             intmcp_episode_root* root, intmcp_episode_kept* kept,
                             const double* pow_table, int32_t max_steps, int32_t until,
                             const pomcp_episode_population* pop,
                             const pomcp_episode_pop_state* ps, pomcp_episode_state* st,
                             pomcp_episode_step_out* out, int32_t* next_action) {
  if (!episode_env_ok(env_id, grid, ego) || !root || !kept || !pow_table || !st || !out ||
      !next_action || max_steps < 1 ||
      (until != POMCP_UNTIL_AGENT_DONE && until != POMCP_UNTIL_ALL_DONE))
    return POMCP_E_INVALID;
  EpPopTables t;
  if (pop) {
    if (!ps || !ep_pop_tables(*pop, host_env_actions(env_id), &t) ||
        ps->policy_index < 0 || ps->policy_index >= t.n)
      return POMCP_E_INVALID;
  }
  const EpPopTables* tp = pop ? &t : nullptr;
  const int k = pop ? ps->policy_index : -1;
  int parked = 0;
  with_host_env(env_id, grid, [&](auto e, const auto& m) {
    *next_action = im_episode_step<decltype(e)>(m, ego, root, kept, pow_table, max_steps, until, tp,
                                                k, st, out, &parked);
  });
  return POMCP_OK;
}

int intmcp_host_episode_unpark(intmcp_episode_root* root, intmcp_episode_kept* kept,
                               int32_t* changed) {
  if (!root || !kept || !changed) return POMCP_E_INVALID;
  *changed = im_episode_unpark(root, kept);
  return POMCP_OK;
}

// k_im_queue_refill's decision per slot (intmcp_episode.h im_episode_refill).
int intmcp_host_episode_refill(int32_t assign, intmcp_episode_kept* kept, int32_t* next_action,
                               int32_t* refilled) {
  if (!kept || !next_action || !refilled || assign < kQueuePlaying) return POMCP_E_INVALID;
  *refilled = im_episode_refill(assign, kept, next_action);
  return POMCP_OK;
}

// The arithmetic k_episode_belief_acc does on a played tree's counts
// (belief_stats.h bel_accuracy).
int pomcp_host_belief_acc(const pomcp_belief_counts* counts, int32_t mixture_index,
                          int32_t other_action, const double* other_pi, int32_t num_other,
                          double out[3]) {
  if (!counts || !out || num_other < 0 || num_other > POMCP_MAX_TYPE_POLICIES ||
      (num_other > 0 && !other_pi) || counts->belief_size < 0)
    return POMCP_E_INVALID;
  bel_accuracy(counts->belief_size, counts->state_matches < 0 ? 0 : counts->state_matches,
               counts->policy_hist, num_other, mixture_index, other_action, other_pi,
               POMCP_MAX_ACTIONS, out);
  return POMCP_OK;
}

// ------------------------------------------------------- host episode queue

// k_log_drop's decision per record (episode_queue.h log_drop_keeps), the kept
// records moved down in order.
int pomcp_host_log_drop(uint32_t* ids, uint32_t* v0, uint32_t* v1, uint32_t* aux, int64_t n,
                        uint64_t lane_mask, int64_t* count_out) {
  if (n < 0 || !count_out || (n > 0 && (!ids || !v0 || !v1))) return POMCP_E_INVALID;
  int64_t out = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (!log_drop_keeps(ids[i], lane_mask)) continue;
    if (out != i) {
      ids[out] = ids[i];
      v0[out] = v0[i];
      v1[out] = v1[i];
      if (aux) aux[out] = aux[i];
    }
    ++out;
  }
  *count_out = out;
  return POMCP_OK;
}

// k_queue_rank's decisions (episode_queue.h), the slots in ascending order.
int pomcp_host_queue_assign(const int32_t* queue_index, const int32_t* finished,
                            int32_t num_slots, int32_t n, int32_t* next_io, int32_t* assign_out,
                            int32_t* refilled_out) {
  if (!queue_index || !finished || !next_io || !assign_out || !refilled_out || num_slots < 1 ||
      n < num_slots || *next_io < num_slots || *next_io > n)
    return POMCP_E_INVALID;
  const int32_t next = *next_io;
  int32_t done = 0;
  for (int32_t b = 0; b < num_slots; ++b) {
    const bool f = queue_slot_finished(queue_index[b], finished[b]);
    assign_out[b] = f ? queue_assign(done, next, n) : kQueuePlaying;
    done += f ? 1 : 0;
  }
  const int32_t r = queue_refilled(done, next, n);
  *next_io = next + r;
  *refilled_out = r;
  return POMCP_OK;
}

// k_group_queue_trees' drop masks (episode_group_queue.h): assign = k_queue_rank's
// decisions for the G groups of K trees each, one mask per search wave.
int pomcp_host_group_drop_masks(const int32_t* assign, int32_t num_groups, int32_t group,
                                int32_t num_trees, uint64_t* masks_out) {
  if (!assign || !masks_out || num_groups < 1 || group < 1 ||
      (int64_t)num_groups * group != num_trees)
    return POMCP_E_INVALID;
  for (int32_t g = 0; g < num_groups; ++g)
    if (assign[g] < kQueuePlaying) return POMCP_E_INVALID;
  const int32_t waves = (num_trees + kGroupQueueWave - 1) / kGroupQueueWave;
  for (int32_t w = 0; w < waves; ++w) masks_out[w] = group_wave_drop_mask(assign, group, num_trees, w);
  return POMCP_OK;
}

// Debug: the same host_exp on the host CPU (tests/test_host_exp.py compares it
// with math.exp without a GPU).
int pomcp_debug_host_exp(const double* x, int32_t n, double* out) {
  if (!x || !out || n < 0) return POMCP_E_INVALID;
  for (int32_t i = 0; i < n; ++i) out[i] = host_exp(x[i]);
  return POMCP_OK;
}

}  // extern "C"
