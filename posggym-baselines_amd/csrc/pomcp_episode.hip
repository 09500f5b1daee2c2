// Batched episodes on the device (pomcp_episodes_begin / _step, pomcp.h): the
// environment side of run_planning_exp (baseline_exps/exp_utils.py:468-552)
// for every tree of a batch at once, between the search and the next update.
//
// One tree per lane (a step is a few hundred instructions and ~100 bytes per
// tree), 256-lane workgroups, the model staged in LDS as the k_synthetic_*
// kernels do.  The per-tree work is episode_step.h's episode_reset /
// episode_step, the code the host twins run.
//
// k_episode_reset  writes  ep.st[b] (cleared, initial state drawn), in_obs[b]
//                  (the ego's initial observation), in_actions[b] = -1, the
//                  query state ep.states[b] when tracked, and ep.ps[b]: the
//                  policy of the population (ep.pop) the tree's other agent
//                  plays this episode, {-1, -1} without one.
// k_episode_step   reads   hdr[b].root_abs / .error (after this step's update),
//                  stats[b] (this step's search), ep.st[b], ep.pow_table, and
//                  with a population its tables and ep.ps[b].policy_index;
//                  writes  ep.st[b], in_obs[b] / in_actions[b] (the next update's
//                  inputs), ep.states[b] when tracked (the state before the
//                  joint action: the one the root belief is about), and for a
//                  tree that finishes hdr[b].root_abs = 1 -- the park: every
//                  kernel leaves a tree with an absorbing root alone
//                  (k_reroot_child, k_compact without a wanted child, k_update,
//                  both search kernels).  A search still rewrites stats[b] of
//                  an absorbing root (zero children), so the record of a tree's
//                  last real search is kept in ep.kept[b] and written back to
//                  stats[b] of a finished tree after every later search.
//                  Unfinished trees and trees with an error are counted per
//                  workgroup (ep.part), k_episode_live adds the counts up:
//                  integers, no atomics, the same on every run.
// Plain C++ and vector stores only.  Included by pomcp_capi.hip.
#pragma clang fp contract(off)

#include "envs.h"
#include "episode_step.h"
#include "pomcp_device.h"

namespace pb {

constexpr int kEpThreads = 256;

struct EpDev {
  pomcp_episode_state* st;        // [B]
  pomcp_root_stats* kept;         // [B] root statistics of each tree's last real search
  const uint64_t* env_seeds;      // [B] (k_episode_reset)
  const double* pow_table;        // [max_steps] discount ** t, the host's
  int32_t* in_actions;            // [B] DevParams::in_actions
  uint64_t* in_obs;               // [B] DevParams::in_obs
  uint2* states;                  // [B] pomcp_belief_stats' query states, or null
  int32_t* part;                  // [workgroups][2] {unfinished, errors}
  int32_t* out;                   // [2] their sums
  int32_t max_steps, until;
  // the other agents' population (pomcp_episodes_set_population): its draw
  // tables, or null for the uniform agent, and every tree's record
  const EpPopTables* pop;
  pomcp_episode_pop_state* ps;    // [B], or null
  // k_episode_belief_acc's error flags, one per workgroup (null: not tracking)
  const int32_t* acc_part;
  int32_t acc_nparts;
};

static_assert(sizeof(pomcp_episode_result) == 80, "episode result layout");
static_assert(sizeof(pomcp_episode_state) == 120, "episode state layout");
static_assert(sizeof(pomcp_root_stats) % 16 == 0, "root stats are copied as 16 B words");

template <class E>
__global__ __launch_bounds__(kEpThreads) void k_episode_reset(DevParams p, EpDev ep) {
  __shared__ typename E::Model sm;
  stage_model(p.model, sm);
  const int b = (int)(blockIdx.x * kEpThreads + threadIdx.x);
  if (b >= p.B) return;
  pomcp_episode_state s;
  pomcp_episode_pop_state r;
  const uint64_t key = episode_reset<E>(sm, p.ego, ep.env_seeds[b], ep.pop, &s, &r);
  ep.st[b] = s;
  if (ep.ps != nullptr) ep.ps[b] = r;
  ep.in_obs[b] = key;
  ep.in_actions[b] = -1;
  if (ep.states != nullptr) ep.states[b] = make_uint2(s.v0, s.v1);
}

template <class E>
__global__ __launch_bounds__(kEpThreads) void k_episode_step(DevParams p, EpDev ep) {
  __shared__ typename E::Model sm;
  stage_model(p.model, sm);
  const int b = (int)(blockIdx.x * kEpThreads + threadIdx.x);
  int live = 0, bad = 0;
  if (b < p.B) {
    pomcp_episode_state s = ep.st[b];
    uint4* const so = reinterpret_cast<uint4*>(p.stats + b);
    uint4* const ko = reinterpret_cast<uint4*>(ep.kept + b);
    constexpr int kW = (int)(sizeof(pomcp_root_stats) / 16);
    if (s.finished) {
      // parked: this step's search saw an absorbing root and zeroed the record
      if (s.res.error == 0)
        for (int k = 0; k < kW; ++k) so[k] = ko[k];
    } else {
      const pomcp_root_stats* const rs = p.stats + b;
      pomcp_episode_step_in in;
      in.root_absorbing = p.hdr[b].root_abs;
      in.error = p.hdr[b].error != 0 ? p.hdr[b].error : rs->error;
      in.action = rs->action;
      in.search_depth = rs->search_depth;
      in.num_sims = rs->num_sims;
      in.pad = 0;
      in.min_value = rs->min_value;
      in.max_value = rs->max_value;
      const bool real = s.root_absorbing == 0 && in.root_absorbing == 0 && in.error == 0;
      if (real)
        for (int k = 0; k < kW; ++k) ko[k] = so[k];
      const uint32_t q0 = s.v0, q1 = s.v1;
      pomcp_episode_step_out out;
      episode_step<E>(sm, p.ego, in, ep.pow_table, ep.max_steps, ep.until, ep.pop,
                      ep.pop != nullptr ? ep.ps[b].policy_index : -1, &s, &out);
      ep.st[b] = s;
      if (out.stepped) {
        ep.in_obs[b] = out.obs_key;
        ep.in_actions[b] = out.ego_action;
        if (ep.states != nullptr) ep.states[b] = make_uint2(q0, q1);
      }
      if (s.finished && s.res.error == 0) {
        p.hdr[b].root_abs = 1;
        if (!real)
          for (int k = 0; k < kW; ++k) so[k] = ko[k];
      }
    }
    live = s.finished ? 0 : 1;
    bad = s.res.error != 0 ? 1 : 0;
  }
  const int nl = __syncthreads_count(live);
  const int nb = __syncthreads_count(bad);
  if (threadIdx.x == 0) {
    ep.part[2 * blockIdx.x] = nl;
    ep.part[2 * blockIdx.x + 1] = nb;
  }
}

// The per-workgroup counts added up by one workgroup, in a fixed order.
__global__ __launch_bounds__(kEpThreads) void k_episode_live(EpDev ep, int nparts) {
  __shared__ int32_t red[2][kEpThreads];
  int32_t a = 0, e = 0;
  for (int i = (int)threadIdx.x; i < nparts; i += kEpThreads) {
    a += ep.part[2 * i];
    e += ep.part[2 * i + 1];
  }
  if (ep.acc_part != nullptr)   // a belief accuracy record with an error counts as one
    for (int i = (int)threadIdx.x; i < ep.acc_nparts; i += kEpThreads) e += ep.acc_part[i];
  red[0][threadIdx.x] = a;
  red[1][threadIdx.x] = e;
  __syncthreads();
  for (int d = kEpThreads / 2; d >= 1; d >>= 1) {
    if ((int)threadIdx.x < d) {
      red[0][threadIdx.x] += red[0][threadIdx.x + d];
      red[1][threadIdx.x] += red[1][threadIdx.x + d];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    ep.out[0] = red[0][0];
    ep.out[1] = red[1][0];
  }
}

}  // namespace pb
