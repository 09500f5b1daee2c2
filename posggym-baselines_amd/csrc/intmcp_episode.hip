// Batched I-NTMCP episodes on the device (intmcp_episodes_begin / _step,
// intmcp.h): pomcp_episode.hip for planner pairs.  One pair per lane, 256-lane
// workgroups, the model staged in LDS; the environment side is episode_step.h's
// episode_reset / episode_step and the I-NTMCP side intmcp_episode.h's
// im_episode_step / im_episode_unpark, the code the host twins run.
//
// k_im_episode_reset   after intmcp_reset's launches; writes ep.st[b] (cleared,
//                      initial state drawn), ep.ps[b] (the population's draw),
//                      in_obs[b] (the ego's initial observation) and
//                      in_actions[b] = -1.
// k_im_episode_step    after the search; reads of pair b the header fields and
//                      the root node word k_im_root_stats reads (last_action,
//                      num_sims, search_depth, err, mm_min / mm_max[T], the
//                      info word of node N(T, cur), T = nest0 ? 1 : 0), ep.st[b],
//                      kept[b]; writes ep.st[b], kept[b], the next update's
//                      in_obs[b] / in_actions[b], and for a pair that finishes
//                      the park: in_actions[b] = INTMCP_SKIP and the absorbing
//                      bit of its root node's info word.  Unfinished pairs and
//                      pairs with an error are counted per workgroup (ep.part);
//                      k_episode_live (pomcp_episode.hip) adds the counts up.
// k_im_episode_unpark  when the batch ends: a parked pair's root info word and
//                      its header's last_action / num_sims / search_depth as
//                      its last real step left them; a second launch changes
//                      nothing.
// Plain C++ and vector stores only.  Included by pomcp_capi.hip after intmcp.hip.
#pragma clang fp contract(off)

#include "intmcp_episode.h"

namespace pb {

static_assert(kImEpSkip == kImSkip, "the update's skip action");
static_assert(sizeof(intmcp_episode_root) == 40, "episode root layout");
static_assert(sizeof(intmcp_episode_kept) == 32, "episode side record layout");

// the planning agent as the environment knows it (ImParams::ego is the agent
// of tree 0, the other agent's at nesting level 0)
__device__ __forceinline__ int im_episode_ego(const ImParams& p) { return p.nest0 ? p.other : p.ego; }

// pair b's planner root: the info word of node N(T, cur)
__device__ __forceinline__ uint32_t* im_episode_root_info(const ImParams& p, int b, int cur) {
  const int T = p.nest0 ? 1 : 0;
  char* const line = p.nodes + im_node_off(p.Nn, p.B, b, T, cur, p.nt);
  return &reinterpret_cast<INode*>(line)->info;
}

template <class E>
__global__ __launch_bounds__(kEpThreads) void k_im_episode_reset(ImParams p, EpDev ep,
                                                                 intmcp_episode_kept* kept) {
  __shared__ typename E::Model sm;
  stage_model(p.model, sm);
  const int b = (int)(blockIdx.x * kEpThreads + threadIdx.x);
  if (b >= p.B) return;
  pomcp_episode_state s;
  pomcp_episode_pop_state r;
  const uint64_t key = episode_reset<E>(sm, im_episode_ego(p), ep.env_seeds[b], ep.pop, &s, &r);
  ep.st[b] = s;
  ep.ps[b] = r;
  ep.in_obs[b] = key;
  ep.in_actions[b] = -1;
  intmcp_episode_kept k;
  k.info = 0u;
  k.last_action = -1;
  k.num_sims = k.search_depth = 0;
  k.parked = 0;
  k.pad[0] = k.pad[1] = k.pad[2] = 0;
  kept[b] = k;
}

template <class E>
__global__ __launch_bounds__(kEpThreads) void k_im_episode_step(ImParams p, EpDev ep,
                                                                intmcp_episode_kept* kept) {
  __shared__ typename E::Model sm;
  stage_model(p.model, sm);
  const int b = (int)(blockIdx.x * kEpThreads + threadIdx.x);
  int live = 0, bad = 0;
  if (b < p.B) {
    pomcp_episode_state s = ep.st[b];
    if (!s.finished) {   // (a finished pair is parked: nothing of it is read or written)
      const IHdr& h = p.hdr[b];
      const int T = p.nest0 ? 1 : 0;
      uint32_t* const info = im_episode_root_info(p, b, h.cur);
      intmcp_episode_root root;
      root.last_action = h.last_action;
      root.num_sims = h.num_sims;
      root.search_depth = h.search_depth;
      root.err = h.err;
      root.min_value = h.mm_min[T];
      root.max_value = h.mm_max[T];
      root.info = *info;
      root.pad = 0;
      intmcp_episode_kept k = kept[b];
      pomcp_episode_step_out out;
      int parked;
      const int32_t next =
          im_episode_step<E>(sm, im_episode_ego(p), &root, &k, ep.pow_table, ep.max_steps, ep.until,
                             ep.pop, ep.pop != nullptr ? ep.ps[b].policy_index : -1, &s, &out, &parked);
      ep.st[b] = s;
      kept[b] = k;
      if (out.stepped) ep.in_obs[b] = out.obs_key;
      if (next != kImEpKeepInput) ep.in_actions[b] = next;
      if (parked) *info = root.info;
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

__global__ __launch_bounds__(kEpThreads) void k_im_episode_unpark(ImParams p,
                                                                  intmcp_episode_kept* kept) {
  const int b = (int)(blockIdx.x * kEpThreads + threadIdx.x);
  if (b >= p.B) return;
  intmcp_episode_kept k = kept[b];
  if (k.parked == 0) return;
  IHdr& h = p.hdr[b];
  uint32_t* const info = im_episode_root_info(p, b, h.cur);
  intmcp_episode_root root;
  root.last_action = h.last_action;
  root.num_sims = h.num_sims;
  root.search_depth = h.search_depth;
  root.err = h.err;
  root.min_value = root.max_value = 0.0;
  root.info = *info;
  root.pad = 0;
  if (im_episode_unpark(&root, &k)) {
    *info = root.info;
    h.last_action = root.last_action;
    h.num_sims = root.num_sims;
    h.search_depth = root.search_depth;
    kept[b] = k;
  }
}

}  // namespace pb
