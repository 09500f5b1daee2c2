// The episode queue of root-parallel planners (pomcp_episodes_group_queue_begin,
// pomcp.h): the queue's slots are the G planner groups of K replica trees each,
// group g = trees [gK, (g+1)K).  The assignment rule is episode_queue.h's with
// "slot" meaning "group" (k_queue_rank over G slots); what is new is how a
// group's decision reaches its K trees and their search waves' drop masks.  One
// implementation for the device kernel (k_group_queue_trees,
// pomcp_episode_group_queue.hip) and its host twin (pomcp_host_group_drop_masks,
// host_api.cpp), so the CPU suite runs the decisions the kernel takes.  Plain
// C++: no HIP dependency.
#ifndef PB_EPISODE_GROUP_QUEUE_H_
#define PB_EPISODE_GROUP_QUEUE_H_
#include <stdint.h>

#include "episode_queue.h"

namespace pb {

constexpr int kGroupQueueWave = 64;   // trees per search wave (pomcp_device.h kWave)

// The group that owns tree b of a batch with K replicas per group.
PB_HD int32_t group_of_tree(int32_t b, int32_t K) { return b / K; }

// Is tree b reset for a new episode this step?  assign[g] is k_queue_rank's
// decision for group g: an entry (>= 0) refills all K of its trees; a group
// that retires (kQueueRetire) or plays on (kQueuePlaying) leaves them alone.
PB_HD bool group_tree_refilled(const int32_t* assign, int32_t K, int32_t b) {
  return assign[group_of_tree(b, K)] >= 0;
}

// The drop mask of search wave w (trees [64 w, 64 w + 64) below num_trees): bit
// l is tree 64 w + l's decision.  The device forms it with one __ballot of
// group_tree_refilled over the wave's lanes; this is the same OR, lane by lane.
PB_HD uint64_t group_wave_drop_mask(const int32_t* assign, int32_t K, int32_t num_trees, int32_t w) {
  uint64_t m = 0ull;
  for (int32_t l = 0; l < kGroupQueueWave; ++l) {
    const int64_t b = (int64_t)w * kGroupQueueWave + l;
    if (b < num_trees && group_tree_refilled(assign, K, (int32_t)b)) m |= 1ull << l;
  }
  return m;
}

}  // namespace pb

#endif  // PB_EPISODE_GROUP_QUEUE_H_
