// A root-parallel planner's episode, per step: the decisions one GROUP of K
// replica trees takes between the merged search and the next update
// (POMCP.step / update / get_action with MCTSConfig.root_parallel = K,
// planning/pomcp.py; OracleRootParallel, oracle/root_parallel.py).  One
// implementation for the device kernel (k_group_episode_step,
// pomcp_episode_group.hip) and its host twin (pomcp_host_episode_group_step_in,
// host_api.cpp), so the CPU suite runs the code the kernel runs.  Plain C++:
// no HIP dependency.
//
// The replicas are looked at in chunks of kEpGroupChunk (a wave's lanes on the
// device, one __ballot per flag and chunk; a loop on the host).  A chunk is
// summarised as (some replica's root is not absorbing, the first non-zero
// update error, the first non-zero search error) in replica order and the
// chunks are folded in order (ep_group_fold), so the group's error is the
// first non-zero update error in replica order, or without one the first
// non-zero search error: the order pomcp_update / pomcp_search report them in.
#ifndef PB_EPISODE_GROUP_H_
#define PB_EPISODE_GROUP_H_
#include <stdint.h>

#include "philox.h"   // PB_HD
#include "../../include/pomcp.h"

namespace pb {

constexpr int kEpGroupChunk = 64;

struct EpGroupFlags {
  int32_t any_live;       // some replica's root is not absorbing
  int32_t update_error;   // first non-zero, replica order
  int32_t search_error;   // first non-zero, replica order
};

PB_HD EpGroupFlags ep_group_none() { return EpGroupFlags{0, 0, 0}; }

// acc: the chunks before this one; c: this chunk's summary.
PB_HD void ep_group_fold(EpGroupFlags* acc, const EpGroupFlags& c) {
  acc->any_live |= c.any_live;
  if (acc->update_error == 0) acc->update_error = c.update_error;
  if (acc->search_error == 0) acc->search_error = c.search_error;
}

// The planner's part of episode_step (episode_step.h) for a group of K
// replicas that searched num_sims simulations each, from the folded flags and
// the group's merged record (k_merge_roots):
//   * the planner's root is absorbing only when every replica's is;
//   * the played action is the merged one; a step whose update made every
//     replica absorbing reaches the statistics with action 0, depth 0 and no
//     simulation (get_action returns action_space[0], mcts.py:270-272);
//   * any other step reports K * num_sims simulations whatever its individual
//     replicas did (POMCP._search returns per_replica * K), the merged maximum
//     depth, and the merged minimum / maximum of the replicas' MinMaxStats.
PB_HD void ep_group_step_in(const EpGroupFlags& f, const pomcp_merged_root& m, int K, int num_sims,
                            pomcp_episode_step_in* in) {
  const int absorbing = f.any_live ? 0 : 1;
  in->root_absorbing = absorbing;
  in->error = f.update_error != 0 ? f.update_error : f.search_error;
  in->action = absorbing ? 0 : m.action;
  in->search_depth = absorbing ? 0 : m.search_depth;
  in->num_sims = absorbing ? 0 : K * num_sims;
  in->pad = 0;
  in->min_value = m.min_value;
  in->max_value = m.max_value;
}

// The merged record of this step is the one to keep (the group's last real
// step): the planner searched, i.e. its root was absorbing neither before nor
// after the update, and nothing failed.
PB_HD bool ep_group_real(int was_absorbing, const pomcp_episode_step_in& in) {
  return was_absorbing == 0 && in.root_absorbing == 0 && in.error == 0;
}

}  // namespace pb

#endif  // PB_EPISODE_GROUP_H_
