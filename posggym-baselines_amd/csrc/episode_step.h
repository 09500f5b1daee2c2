// One tree's episode, per step (run_planning_exp, baseline_exps/exp_utils.py:
// 468-552, against a uniform random other agent): the start of an episode and
// one environment step with its bookkeeping.  One implementation for the
// device kernels (k_episode_reset / k_episode_step, pomcp_episode.hip) and
// their host twins (pomcp_host_episode_reset / pomcp_host_episode_step and
// their _pop forms, host_api.cpp), so the CPU suite and the sanitized host build run the code
// the kernels run.  Plain C++: no HIP dependency.
//
// The environment's draws are those of the serial harness
// (planning/episodes.py, oracle/episode.py): under the key (env seed,
// kEnvTreeKey) the model stream gives the initial state and Driving's
// execution-order shuffle (one draw per step, the counter carried from step to
// step), and stream S_ENV_POLICY_BASE + i gives agent i's uniform action, one
// draw per step.
//
// With a population (EpPopTables, from a pomcp_episode_population) the other
// agent is one of its fixed-distribution policies instead: the reset draws the
// episode's policy as uniform_int(word 0 of stream S_ENV_POPULATION, n) (the
// build's model.rng.choice(ids), UniformOtherAgentFn,
// utils/agent_env_wrapper.py:8-27) and the step turns the same word of the
// agent's stream into an action as CPython's random.choices does
// (PopulationAgents, planning/episodes.py).  A null population is the uniform
// agent, draw for draw.  A member of a reactive kind (pomcp_policy_kinds)
// acts on the true state before the joint action instead (E::policy_draw);
// the word is still taken, so every counter advances as for a fixed member.
// A deterministic kind ignores the word; PredatorPrey's heuristics draw with it.
#ifndef PB_EPISODE_STEP_H_
#define PB_EPISODE_STEP_H_
#include <stdint.h>

#include "cooperative_reaching.h"
#include "driving.h"
#include "driving_policy.h"
#include "philox.h"
#include "predator_prey.h"
#include "predator_prey_policy.h"
#include "pursuit_evasion.h"
#include "../../include/pomcp.h"

// (FP64 sums below: no fused multiply-add, as everywhere in the engine)
#pragma clang fp contract(off)

namespace pb {

constexpr uint32_t kEnvTreeKey = 0x40000000u;

// The environment side of an episode: both agents' rewards and termination
// flags (Env of envs.h gives the search the ego's alone).
struct EpDriving {
  using Model = DrvModel;
  static constexpr uint32_t kA = 5;
  template <class Draw>
  PB_HD static void sample_initial(const Model& m, Draw draw, uint32_t* s0, uint32_t* s1) {
    drv_sample_initial_state2(m.g, draw, s0, s1);
  }
  // pomcp_driving_step: the execution-order shuffle is one model draw
  PB_HD static void step(const Model& m, Streams& env, uint32_t s0, uint32_t s1, int a0, int a1,
                         uint32_t* n0, uint32_t* n1, double r[2], int term[2]) {
    const uint32_t j = env.model(2);
    drv_step2_fast(m, s0, s1, a0, a1, j, n0, n1);
    r[0] = drv_reward_fast(m, s0, *n0);
    r[1] = drv_reward_fast(m, s1, *n1);
    term[0] = veh_done(*n0) ? 1 : 0;
    term[1] = veh_done(*n1) ? 1 : 0;
  }
  PB_HD static uint64_t obs_key(const Model& m, int agent, uint32_t n0, uint32_t n1) {
    return agent == 0 ? obs_key_fast(m, n0, n1) : obs_key_fast(m, n1, n0);
  }
  PB_HD static bool has_kind(int kind) { return kind == POMCP_POLICY_DRIVING_SHORTEST_PATH; }
  // the action of `agent` under a reactive kind in the state (s0, s1)
  PB_HD static int policy_action(const Model& m, int agent, uint32_t s0, uint32_t s1, int /*kind*/,
                                 int p0, int p1) {
    return drv_sp_action(m.g, agent == 0 ? s0 : s1, agent == 0 ? s1 : s0, p0, p1);
  }
  // the same with the word of the agent's stream (a stochastic kind draws with it)
  PB_HD static int policy_draw(const Model& m, int agent, uint32_t s0, uint32_t s1, int kind, int p0,
                               int p1, uint32_t /*w*/) {
    return policy_action(m, agent, s0, s1, kind, p0, p1);
  }
};

struct EpPursuitEvasion {
  using Model = PeModel;
  static constexpr uint32_t kA = 4;
  template <class Draw>
  PB_HD static void sample_initial(const Model& m, Draw draw, uint32_t* s0, uint32_t* s1) {
    pe_sample_initial_state(m, draw, s0, s1);
  }
  // pomcp_pe_step: deterministic, both agents terminate together
  PB_HD static void step(const Model& m, Streams& /*env*/, uint32_t s0, uint32_t s1, int a0, int a1,
                         uint32_t* n0, uint32_t* n1, double r[2], int term[2]) {
    uint32_t prog, outcome;
    pe_step(m, s0, s1, (uint32_t)a0, (uint32_t)a1, n0, n1, &prog, &outcome);
    r[0] = pe_reward(m, 0, s0, prog, outcome);
    r[1] = pe_reward(m, 1, s0, prog, outcome);
    term[0] = term[1] = pe_done(*n0) ? 1 : 0;
  }
  PB_HD static uint64_t obs_key(const Model& m, int agent, uint32_t n0, uint32_t n1) {
    return pe_obs_key(m, agent, n0, n1);
  }
  // (no reactive kinds: a population with one is refused before it gets here)
  PB_HD static bool has_kind(int /*kind*/) { return false; }
  PB_HD static int policy_action(const Model&, int, uint32_t, uint32_t, int, int, int) { return 0; }
  PB_HD static int policy_draw(const Model& m, int agent, uint32_t s0, uint32_t s1, int kind, int p0,
                               int p1, uint32_t /*w*/) {
    return policy_action(m, agent, s0, s1, kind, p0, p1);
  }
};

struct EpCoopReaching {
  using Model = CrModel;
  static constexpr uint32_t kA = 5;
  template <class Draw>
  PB_HD static void sample_initial(const Model& m, Draw draw, uint32_t* s0, uint32_t* s1) {
    cr_sample_initial_state(m, draw, s0, s1);
  }
  // pomcp_cr_step: deterministic, one reward for both, both terminate together
  PB_HD static void step(const Model& m, Streams& /*env*/, uint32_t s0, uint32_t s1, int a0, int a1,
                         uint32_t* n0, uint32_t* n1, double r[2], int term[2]) {
    cr_step(m, s0, s1, (uint32_t)a0, (uint32_t)a1, n0, n1, &r[0]);
    r[1] = r[0];
    term[0] = term[1] = cr_done(*n0, *n1) ? 1 : 0;
  }
  PB_HD static uint64_t obs_key(const Model& m, int agent, uint32_t n0, uint32_t n1) {
    return cr_obs_key(m, agent, n0, n1);
  }
  PB_HD static bool has_kind(int kind) { return kind == POMCP_POLICY_CR_GOAL; }
  PB_HD static int policy_action(const Model& m, int agent, uint32_t s0, uint32_t s1, int /*kind*/,
                                 int p0, int /*p1*/) {
    return cr_goal_action(m, agent == 0 ? s0 : s1, p0);
  }
  PB_HD static int policy_draw(const Model& m, int agent, uint32_t s0, uint32_t s1, int kind, int p0,
                               int p1, uint32_t /*w*/) {
    return policy_action(m, agent, s0, s1, kind, p0, p1);
  }
};

struct EpPredatorPrey {
  using Model = PpModel;
  static constexpr uint32_t kA = 5;
  static constexpr uint32_t kStepRange = kPpStepRange;
  template <class Draw>
  PB_HD static void sample_initial(const Model& m, Draw draw, uint32_t* s0, uint32_t* s1) {
    pp_sample_initial_state(m, draw, s0, s1);
  }
  // pomcp_pp_step: the prey's tie bytes and the predators' order are one model
  // draw; one reward for both, both terminate together
  PB_HD static void step(const Model& m, Streams& env, uint32_t s0, uint32_t s1, int a0, int a1,
                         uint32_t* n0, uint32_t* n1, double r[2], int term[2]) {
    const uint32_t j = env.model(kStepRange);
    pp_step(m, s0, s1, (uint32_t)a0, (uint32_t)a1, j, n0, n1, &r[0]);
    r[1] = r[0];
    term[0] = term[1] = pp_done(*n0) ? 1 : 0;
  }
  PB_HD static uint64_t obs_key(const Model& m, int agent, uint32_t n0, uint32_t n1) {
    return pp_obs_key(m, agent, n0, n1);
  }
  // the heuristic agents H1 .. H3 (predator_prey_policy.h): a distribution that
  // depends on the state, drawn with the word of the agent's stream
  PB_HD static bool has_kind(int kind) { return kind == POMCP_POLICY_PP_HEURISTIC; }
  PB_HD static int policy_draw(const Model& m, int agent, uint32_t s0, uint32_t s1, int /*kind*/,
                               int p0, int /*p1*/, uint32_t w) {
    return pp_heuristic_action(m, agent, s0, s1, p0, w);
  }
};

// kind / parameters of one policy of a population or a mixture
// (pomcp_policy_kinds), whichever environment has the kind: false for an
// unknown kind or a parameter out of range.
PB_HD bool policy_kind_ok(int kind, int p0, int p1) {
  return drv_policy_kind_ok(kind, p0, p1) || cr_policy_kind_ok(kind, p0, p1) ||
         pp_policy_kind_ok(kind, p0, p1);
}

// A population's draw tables: random.choices' cumulative weights
// (itertools.accumulate) and total = cum[-1] + 0.0 per policy
// (planning/policies.py cumulative), the doubles Python bisects.
struct EpPopTables {
  int32_t n, pad;
  double cum[POMCP_MAX_TYPE_POLICIES][POMCP_MAX_ACTIONS];
  double tot[POMCP_MAX_TYPE_POLICIES];
  int32_t mix[POMCP_MAX_TYPE_POLICIES];
  // pomcp_policy_kinds: POMCP_POLICY_FIXED draws from cum / tot, a reactive
  // kind acts by E::policy_draw(kind, p0, p1, word)
  int32_t kind[POMCP_MAX_TYPE_POLICIES];
  int32_t p0[POMCP_MAX_TYPE_POLICIES], p1[POMCP_MAX_TYPE_POLICIES];
};

// false: not 1..8 policies, a negative (or NaN) probability, or a zero sum.
inline bool ep_pop_tables(const pomcp_episode_population& p, int A, EpPopTables* t) {
  if (p.num_policies < 1 || p.num_policies > POMCP_MAX_TYPE_POLICIES || A < 1 ||
      A > POMCP_MAX_ACTIONS)
    return false;
  *t = EpPopTables{};
  t->n = p.num_policies;
  for (int k = 0; k < p.num_policies; ++k) {
    double acc = 0.0;
    for (int a = 0; a < A; ++a) {
      if (!(p.pi[k][a] >= 0.0)) return false;
      acc = a == 0 ? p.pi[k][a] : acc + p.pi[k][a];
      t->cum[k][a] = acc;
    }
    t->tot[k] = acc + 0.0;
    if (!(t->tot[k] > 0.0)) return false;
    t->mix[k] = p.mixture_index[k];
  }
  return true;
}

// The kinds of a population's policies into its tables (null: all fixed).
// POMCP_E_UNSUPPORTED: a reactive kind the environment E does not have;
// POMCP_E_INVALID: an unknown kind or a parameter out of range.
template <class E>
inline int ep_pop_kinds(const pomcp_policy_kinds* kinds, EpPopTables* t) {
  for (int k = 0; k < POMCP_MAX_TYPE_POLICIES; ++k) t->kind[k] = t->p0[k] = t->p1[k] = 0;
  if (kinds == nullptr) return POMCP_OK;
  for (int k = 0; k < t->n; ++k) {
    if (!policy_kind_ok(kinds->kind[k], kinds->param0[k], kinds->param1[k]))
      return POMCP_E_INVALID;
    if (kinds->kind[k] != POMCP_POLICY_FIXED && !E::has_kind(kinds->kind[k]))
      return POMCP_E_UNSUPPORTED;
  }
  for (int k = 0; k < t->n; ++k) {
    t->kind[k] = kinds->kind[k];
    t->p0[k] = kinds->param0[k];
    t->p1[k] = kinds->param1[k];
  }
  return POMCP_OK;
}

// random.choices(range(n), weights): bisect_right(cum, x, 0, n - 1) for
// x = random() * total (tm_choice of pomcp_device.h, for host and device).
PB_HD int ep_choice(const double* cum, double total, int n, uint32_t w) {
  const double x = uniform_float(w) * total;
  int i = n - 1;
  for (int q = n - 2; q >= 0; --q)
    if (x < cum[q]) i = q;
  return i;
}

PB_HD Streams episode_streams(const pomcp_episode_state& st) {
  Streams env;
  env.seed = st.res.env_seed;
  env.tree = kEnvTreeKey;
  for (int k = 0; k < 5; ++k) env.ctr[k] = 0;
  env.ctr[2] = st.model_ctr;
  return env;
}

// A fresh episode under env_seed: the record cleared, the initial state drawn;
// returns the ego's initial observation.
template <class E>
PB_HD uint64_t episode_reset(const typename E::Model& m, int ego, uint64_t env_seed,
                             pomcp_episode_state* st) {
  pomcp_episode_state s;
  s.res.env_seed = env_seed;
  s.res.len = 0;
  s.res.searched_steps = 0;
  s.res.ret = 0.0;
  s.res.discounted_return = 0.0;
  s.res.ego_terminated = s.res.all_done = s.res.truncated = 0;
  s.res.error = 0;
  s.res.search_depth_sum = 0;
  s.res.num_sims_sum = 0;
  s.res.min_value_sum = 0.0;
  s.res.max_value_sum = 0.0;
  s.model_ctr = 0u;
  s.policy_ctr = 0u;
  s.last_action = -1;
  s.finished = 0;
  s.root_absorbing = 0;
  s.last_other_action = -1;
  s.last_reward = 0.0;
  Streams env = episode_streams(s);
  E::sample_initial(m, [&](uint32_t n) { return env.model(n); }, &s.v0, &s.v1);
  s.model_ctr = env.ctr[2];
  *st = s;
  return E::obs_key(m, ego, s.v0, s.v1);
}

// The same with a population (null: no draw, ps = {-1, -1}): the episode's
// policy index and its mixture index go to *ps.
template <class E>
PB_HD uint64_t episode_reset(const typename E::Model& m, int ego, uint64_t env_seed,
                             const EpPopTables* pop, pomcp_episode_state* st,
                             pomcp_episode_pop_state* ps) {
  pomcp_episode_pop_state r;
  r.policy_index = r.mixture_index = -1;
  if (pop != nullptr) {
    r.policy_index = (int32_t)uniform_int(
        philox_word(env_seed, kEnvTreeKey, (uint32_t)S_ENV_POPULATION, 0u), (uint32_t)pop->n);
    r.mixture_index = pop->mix[r.policy_index];
  }
  *ps = r;
  return episode_reset<E>(m, ego, env_seed, st);
}

// One step of an unfinished episode (out->stepped = 0 and nothing changes for a
// finished one).  The planner's part is `in`; pow_table[t] = discount ** t has
// max_steps entries.
// pop / policy_index: the population and the episode's policy (null: uniform).
template <class E>
PB_HD void episode_step(const typename E::Model& m, int ego, const pomcp_episode_step_in& in,
                        const double* pow_table, int max_steps, int until, const EpPopTables* pop,
                        int policy_index, pomcp_episode_state* st, pomcp_episode_step_out* out) {
  pomcp_episode_state s = *st;
  out->obs_key = 0ull;
  out->reward = 0.0;
  out->ego_action = out->other_action = -1;
  out->stepped = 0;
  out->pad = 0;
  if (s.finished) return;
  if (in.error != 0 || s.res.len >= max_steps) {   // (the second: a record no step leaves)
    s.res.error = in.error != 0 ? in.error : POMCP_E_STATE;
    s.finished = 1;
    *st = s;
    return;
  }
  // planner.step (mcts.py:97-117): a root that was absorbing before this step
  // returns the last action and records nothing; any other step reaches the
  // statistics, also the one whose update made the root absorbing (get_action
  // returns action_space[0] with no simulation then, mcts.py:270-272)
  const bool tracked = s.root_absorbing == 0;
  int a_ego = tracked ? in.action : s.last_action;
  if (a_ego < 0 || a_ego >= (int)E::kA) a_ego = 0;
  if (tracked) {
    s.res.searched_steps += 1;
    s.res.search_depth_sum += in.search_depth;
    s.res.num_sims_sum += in.num_sims;
    s.res.min_value_sum = s.res.min_value_sum + in.min_value;
    s.res.max_value_sum = s.res.max_value_sum + in.max_value;
  }
  s.root_absorbing = in.root_absorbing;
  // UniformRandomAgents.act (planning/episodes.py:85-92): draw j of the agent's stream
  const int other = 1 - ego;
  // (PopulationAgents.act: the same word through the policy's bisection)
  const uint32_t w_oth = philox_word(s.res.env_seed, kEnvTreeKey,
                                     (uint32_t)S_ENV_POLICY_BASE + (uint32_t)other, s.policy_ctr);
  int a_oth;
  if (pop != nullptr) {
    const int k = policy_index >= 0 && policy_index < pop->n ? policy_index : 0;
    if (pop->kind[k] != POMCP_POLICY_FIXED)
      a_oth = E::policy_draw(m, other, s.v0, s.v1, pop->kind[k], pop->p0[k], pop->p1[k], w_oth);
    else
      a_oth = ep_choice(pop->cum[k], pop->tot[k], (int)E::kA, w_oth);
  } else {
    a_oth = (int)uniform_int(w_oth, E::kA);
  }
  s.policy_ctr += 1u;
  Streams env = episode_streams(s);
  uint32_t n0, n1;
  double r[2];
  int term[2];
  E::step(m, env, s.v0, s.v1, ego == 0 ? a_ego : a_oth, ego == 0 ? a_oth : a_ego, &n0, &n1, r,
          term);
  s.model_ctr = env.ctr[2];
  const double reward = r[ego];
  s.res.ret = s.res.ret + reward;
  const double disc = pow_table[s.res.len] * reward;
  s.res.discounted_return = s.res.discounted_return + disc;
  s.res.len += 1;
  s.v0 = n0;
  s.v1 = n1;
  s.last_action = a_ego;
  s.last_other_action = a_oth;
  s.last_reward = reward;
  const int all = term[0] && term[1] ? 1 : 0;
  s.res.ego_terminated = term[ego];
  s.res.all_done = all;
  s.res.truncated = s.res.len >= max_steps ? 1 : 0;
  // planning/episodes.py:148-153
  const int done = until == POMCP_UNTIL_AGENT_DONE ? (term[ego] | all) : all;
  s.finished = (done | s.res.truncated) ? 1 : 0;
  *st = s;
  out->obs_key = E::obs_key(m, ego, n0, n1);
  out->reward = reward;
  out->ego_action = a_ego;
  out->other_action = a_oth;
  out->stepped = 1;
}

template <class E>
PB_HD void episode_step(const typename E::Model& m, int ego, const pomcp_episode_step_in& in,
                        const double* pow_table, int max_steps, int until,
                        pomcp_episode_state* st, pomcp_episode_step_out* out) {
  episode_step<E>(m, ego, in, pow_table, max_steps, until, nullptr, -1, st, out);
}

}  // namespace pb

#endif  // PB_EPISODE_STEP_H_
