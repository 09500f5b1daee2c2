// The episode queue of root-parallel planners (pomcp_episodes_group_queue_begin,
// pomcp.h): the queue's slots are the G planner groups of a
// batch of G * K trees, and a group whose episode ends takes the next
// environment seed of the device-resident queue.  Launched by
// pomcp_episodes_step while a group queue is active, after k_group_episode_step
// and k_queue_rank (over G slots, unchanged) and before k_log_drop (unchanged)
// and k_episode_live:
//
// k_group_queue_refill  one group per lane: k_queue_refill's work for a slot
//                 that is a group.  A finished group's record goes out to
//                 rows[its entry] and fin[g], its kept merged record to
//                 fin_merged[g] (zeros for a group where no episode ended).
//                 With a new entry the group's one environment starts
//                 (episode_reset, the population policy drawn per group), the
//                 kept merged record is zeroed, slot_ord / slot_start advance
//                 and the new observation key is left in key[g] for the trees.
// k_group_queue_trees   one tree per lane, g = b / K (episode_group_queue.h): a
//                 tree of a refilled group is reset as k_reset resets it but
//                 for the wave's shared log count (queue_reset_tree), takes
//                 in_obs[b] = key[g] and in_actions[b] = -1, and sets its bit
//                 in its search wave's drop mask.  A group's K replicas span
//                 several search waves and several groups share one, so the
//                 masks are formed where the trees are: a 256-lane workgroup
//                 holds four search waves' trees, one per hardware wave, a
//                 mask is one __ballot stored by lane 0, and every wave's mask
//                 is rewritten on every step.  No atomics, no barrier.
// Plain C++ and vector stores only.  Included by pomcp_capi.hip after
// pomcp_episode_group.hip and pomcp_episode_queue.hip.
#pragma clang fp contract(off)

#include "episode_group_queue.h"

namespace pb {

static_assert(kGroupQueueWave == kWave, "a drop mask is one search wave's lanes");
static_assert(sizeof(pomcp_episode_state) % 8 == 0 && sizeof(pomcp_episode_result) % 8 == 0 &&
                  offsetof(pomcp_episode_state, res) == 0 &&
                  offsetof(pomcp_episode_queue_row, res) == 0,
              "a finished record and its result are copied as 8 B words");

struct EpGroupQueueDev {
  uint64_t* key;                   // [G] a refilled group's first observation key
  pomcp_merged_root* fin_merged;   // [G] the kept merged records of the episodes that ended this step
};

template <class E>
__global__ __launch_bounds__(kEpThreads) void k_group_queue_refill(DevParams p, EpDev ep,
                                                                  EpGroupDev gr, EpQueueDev q,
                                                                  EpGroupQueueDev gq) {
  __shared__ typename E::Model sm;
  stage_model(p.model, sm);
  const int g = (int)(blockIdx.x * kEpThreads + threadIdx.x);
  if (g >= gr.G) return;   // (no barrier below)
  constexpr int kMergedWords = (int)(sizeof(pomcp_merged_root) / 16);
  constexpr int kStateWords = (int)(sizeof(pomcp_episode_state) / 8);
  constexpr int kResultWords = (int)(sizeof(pomcp_episode_result) / 8);
  const int32_t a = q.assign[g];
  uint4* const ko = reinterpret_cast<uint4*>(gr.kept + g);
  uint4* const fo = reinterpret_cast<uint4*>(gq.fin_merged + g);
  int32_t fq = -1;
  if (a == kQueuePlaying) {
    for (int w = 0; w < kMergedWords; ++w) fo[w] = make_uint4(0, 0, 0, 0);
  } else {
    const int32_t at = q.slot_q[g];
    fq = at;
    pomcp_episode_queue_row* const row = q.rows + at;
    // the record goes to fin[g] and its result (the record's head) to the row,
    // word by word from one load each: no private copy of the 120 B record
    const uint64_t* const sw = reinterpret_cast<const uint64_t*>(ep.st + g);
    uint64_t* const fw = reinterpret_cast<uint64_t*>(q.fin + g);
    uint64_t* const rw = reinterpret_cast<uint64_t*>(&row->res);
#pragma unroll
    for (int w = 0; w < kStateWords; ++w) {
      const uint64_t v = sw[w];
      fw[w] = v;
      if (w < kResultWords) rw[w] = v;
    }
    for (int w = 0; w < kMergedWords; ++w) fo[w] = ko[w];
    row->slot = g;
    row->slot_order = q.slot_ord[g];
    row->policy_index = ep.ps != nullptr ? ep.ps[g].policy_index : -1;
    row->start_step = q.slot_start[g];
    q.slot_q[g] = a;   // (kQueueRetire: the replicas stay parked as k_group_episode_step left them)
    if (a >= 0) {
      pomcp_episode_state ns;
      pomcp_episode_pop_state r;
      gq.key[g] = episode_reset<E>(sm, p.ego, q.seeds[a], ep.pop, &ns, &r);
      ep.st[g] = ns;
      if (ep.ps != nullptr) ep.ps[g] = r;
      for (int w = 0; w < kMergedWords; ++w) ko[w] = make_uint4(0, 0, 0, 0);
      q.slot_ord[g] += 1;
      q.slot_start[g] = q.step + 1;
    }
  }
  q.fin_q[g] = fq;
}

__global__ __launch_bounds__(kEpThreads) void k_group_queue_trees(DevParams p, EpDev ep,
                                                                 EpQueueDev q, EpGroupQueueDev gq,
                                                                 int K) {
  const int b = (int)(blockIdx.x * kEpThreads + threadIdx.x);
  const int lane = lane_id();
  const int wave0 = uni(b - lane);   // the first tree of this lane's search wave
  if (wave0 >= p.B) return;          // (whole waves leave: the ballots below are complete)
  bool refill = false, wrapped = false;
  if (b < p.B && group_tree_refilled(q.assign, K, b)) {
    refill = true;
    wrapped = queue_reset_tree(p, b);
    ep.in_obs[b] = gq.key[group_of_tree(b, K)];
    ep.in_actions[b] = -1;
  }
  const uint64_t mask = __ballot(refill);
  if (lane == 0) q.drop[wave0 / kWave] = mask;
  // (rare: once in kEpochMask resets of a tree) the wrapped trees' maps, one
  // after the other by the whole wave
  uint64_t wr = __ballot(wrapped);
  while (wr != 0ull) {
    const int l = __builtin_ctzll(wr);
    clear_ovf(p, wave0 + l, lane);
    wr &= wr - 1ull;
  }
}

}  // namespace pb
