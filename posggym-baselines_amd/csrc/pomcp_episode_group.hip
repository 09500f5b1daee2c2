// Batched episodes with root-parallel planners (pomcp_episodes_set_group,
// pomcp.h): planner g of a batch owns the K replica trees [gK, (g+1)K) and
// plays ONE episode.  After the search pomcp_episodes_step merges every group's
// replicas (k_merge_roots, pomcp_kernels.hip: the summation order lives there
// alone) and k_group_episode_step takes the group's decision
// (episode_group.h), steps its one environment (episode_step.h) and hands the
// same (action, observation) to all K replicas.
//
// One wave per group, kEpThreads / 64 groups per workgroup, the model staged in
// LDS as k_episode_step stages it.  K ranges from 2 to over 1,000, so the lanes
// stride over the replicas in chunks of 64:
//   * hdr[b].root_abs / .error (after this step's update) and stats[b].error
//     (this step's search) of the chunk's replicas, one per lane; "some root is
//     not absorbing" and the first non-zero error in replica order are one
//     __ballot each, folded over the chunks in order (ep_group_fold);
//   * lane 0 runs ep_group_step_in and episode_step<E> on the group's record
//     ep.st[g] (and keeps the merged record of a real step in gr.kept[g]);
//   * its answer is broadcast (__shfl from lane 0) and the lanes store
//     in_obs[b] / in_actions[b] of the K replicas, consecutive lanes to
//     consecutive words, and for an episode that finished hdr[b].root_abs = 1
//     on all K replicas: the park (pomcp_episode.hip).
// Every wave reaches stage_model's barrier and both __syncthreads_count calls:
// a wave without a group (the last workgroup) and a parked group skip the work
// between them, nothing returns early.  Unfinished groups and groups with an
// error are counted per workgroup into ep.part; k_episode_live adds them up.
// Plain C++ and vector stores only, no atomics.  Included by pomcp_capi.hip
// after pomcp_episode.hip.
#pragma clang fp contract(off)

#include "episode_group.h"

namespace pb {

constexpr int kEpGroupWaves = kEpThreads / kWave;   // groups per workgroup

struct EpGroupDev {
  const pomcp_merged_root* merged;   // [G] this step's k_merge_roots results
  pomcp_merged_root* kept;           // [G] the merged record of each group's last real step
  int32_t K, G;                      // replicas per group, groups (G * K = DevParams::B)
  int32_t num_sims, pad;             // simulations per replica of this step's search
};

static_assert(kEpGroupChunk == kWave, "a chunk of replicas is a wave's lanes");
static_assert(sizeof(pomcp_merged_root) % 16 == 0, "merged records are copied as 16 B words");

// v of the first lane (lowest replica) where it is non-zero; 0 if none.
__device__ __forceinline__ int ep_first_nonzero(int v) {
  const unsigned long long m = __ballot(v != 0);
  if (m == 0ull) return 0;
  return __shfl(v, __ffsll(m) - 1);
}

__device__ __forceinline__ uint64_t ep_bcast64(uint64_t v) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, 0);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), 0);
  return ((uint64_t)hi << 32) | lo;
}

// k_episode_reset for groups: one initial state per group (ep.st[g], ep.ps[g],
// drawn under ep.env_seeds[g]); its observation and action -1 to the K replicas.
template <class E>
__global__ __launch_bounds__(kEpThreads) void k_group_episode_reset(DevParams p, EpDev ep,
                                                                   EpGroupDev gr) {
  __shared__ typename E::Model sm;
  stage_model(p.model, sm);
  const int lane = lane_id();
  const int g = uni((int)(blockIdx.x * kEpGroupWaves + (threadIdx.x >> 6)));
  if (g >= gr.G) return;   // (no barrier below)
  uint64_t key = 0ull;
  if (lane == 0) {
    pomcp_episode_state s;
    pomcp_episode_pop_state r;
    key = episode_reset<E>(sm, p.ego, ep.env_seeds[g], ep.pop, &s, &r);
    ep.st[g] = s;
    if (ep.ps != nullptr) ep.ps[g] = r;
  }
  key = ep_bcast64(key);
  const int64_t base = (int64_t)g * gr.K;
  for (int k = lane; k < gr.K; k += kWave) {
    ep.in_obs[base + k] = key;
    ep.in_actions[base + k] = -1;
  }
}

template <class E>
__global__ __launch_bounds__(kEpThreads) void k_group_episode_step(DevParams p, EpDev ep,
                                                                  EpGroupDev gr) {
  __shared__ typename E::Model sm;
  stage_model(p.model, sm);
  const int lane = lane_id();
  const int g = uni((int)(blockIdx.x * kEpGroupWaves + (threadIdx.x >> 6)));
  int live = 0, bad = 0;
  if (g < gr.G) {
    const int K = gr.K;
    const int64_t base = (int64_t)g * K;
    const int parked = uni(ep.st[g].finished);
    if (parked) {
      // every replica's root is absorbing since the step that finished the
      // episode: the updates and searches since left the trees alone
      if (lane == 0) bad = ep.st[g].res.error != 0 ? 1 : 0;
    } else {
      EpGroupFlags f = ep_group_none();
      for (int k0 = 0; k0 < K; k0 += kWave) {
        const int k = k0 + lane;
        int not_abs = 0, ue = 0, se = 0;
        if (k < K) {
          not_abs = p.hdr[base + k].root_abs == 0 ? 1 : 0;
          ue = p.hdr[base + k].error;
          se = p.stats[base + k].error;
        }
        EpGroupFlags c;
        c.any_live = __ballot(not_abs != 0) != 0ull ? 1 : 0;
        c.update_error = ep_first_nonzero(ue);
        c.search_error = ep_first_nonzero(se);
        ep_group_fold(&f, c);
      }
      int stepped = 0, action = -1, park = 0;
      uint64_t key = 0ull;
      if (lane == 0) {
        pomcp_episode_state s = ep.st[g];
        pomcp_episode_step_in in;
        ep_group_step_in(f, gr.merged[g], K, gr.num_sims, &in);
        if (ep_group_real(s.root_absorbing, in)) {
          // (16 B words, as k_episode_step copies a tree's root statistics)
          const uint4* const mo = reinterpret_cast<const uint4*>(gr.merged + g);
          uint4* const ko = reinterpret_cast<uint4*>(gr.kept + g);
          for (int w = 0; w < (int)(sizeof(pomcp_merged_root) / 16); ++w) ko[w] = mo[w];
        }
        pomcp_episode_step_out out;
        episode_step<E>(sm, p.ego, in, ep.pow_table, ep.max_steps, ep.until, ep.pop,
                        ep.pop != nullptr ? ep.ps[g].policy_index : -1, &s, &out);
        ep.st[g] = s;
        stepped = out.stepped;
        action = out.ego_action;
        key = out.obs_key;
        park = s.finished && s.res.error == 0 ? 1 : 0;
        live = s.finished ? 0 : 1;
        bad = s.res.error != 0 ? 1 : 0;
      }
      stepped = __shfl(stepped, 0);
      action = __shfl(action, 0);
      park = __shfl(park, 0);
      key = ep_bcast64(key);
      if (stepped)
        for (int k = lane; k < K; k += kWave) {
          ep.in_obs[base + k] = key;
          ep.in_actions[base + k] = action;
        }
      if (park)
        for (int k = lane; k < K; k += kWave) p.hdr[base + k].root_abs = 1;
    }
  }
  const int nl = __syncthreads_count(live);
  const int nb = __syncthreads_count(bad);
  if (threadIdx.x == 0) {
    ep.part[2 * blockIdx.x] = nl;
    ep.part[2 * blockIdx.x + 1] = nb;
  }
}

}  // namespace pb
