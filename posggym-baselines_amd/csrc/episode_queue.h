// The episode queue of a batch of episodes (pomcp_episodes_queue_begin,
// pomcp.h): the per-record and per-slot decisions of its kernels (k_log_drop,
// k_queue_rank, pomcp_episode_queue.hip) and of their host twins
// (pomcp_host_log_drop, pomcp_host_queue_assign, host_api.cpp), so the CPU
// suite runs the decisions the kernels take.  Plain C++: no HIP dependency.
//
// The assignment rule.  Slot b starts with queue entry b and next = B.  At the
// end of a batch step the slots whose episode finished in that step take the
// entries next, next + 1, ... in ascending slot order while entries remain; a
// slot that finds the queue empty is retired.
#ifndef PB_EPISODE_QUEUE_H_
#define PB_EPISODE_QUEUE_H_
#include <stdint.h>

#include "philox.h"   // PB_HD

namespace pb {

// A log record's tree lane is id >> kLogLaneShift (pomcp_device.h kIdBits; the
// device unit asserts they agree).
constexpr int kLogLaneShift = 26;

// What a slot does at the end of a step (queue_assign's result).
constexpr int32_t kQueuePlaying = -2;   // its episode goes on (or the slot was retired before)
constexpr int32_t kQueueRetire = -1;    // finished, and no entry is left

// Does k_log_drop keep the record?  Not when its tree lane is in the mask; a
// deferred record (id & mask >= cut_base) carries the same lane tag.
PB_HD bool log_drop_keeps(uint32_t id, uint64_t lane_mask) {
  return ((lane_mask >> (id >> kLogLaneShift)) & 1ull) == 0ull;
}

// A slot finished this step when it plays an entry (queue_index >= 0) whose
// episode record says so.
PB_HD bool queue_slot_finished(int32_t queue_index, int32_t episode_finished) {
  return queue_index >= 0 && episode_finished != 0;
}

// The entry of the slot that is `rank`-th (from 0) among this step's finished
// slots in ascending slot order, or kQueueRetire; `next` is the first entry
// not handed out and n the queue's length.
PB_HD int32_t queue_assign(int32_t rank, int32_t next, int32_t n) {
  return rank < n - next ? next + rank : kQueueRetire;
}

// The entries handed out to `finished` slots, and the new `next`.
PB_HD int32_t queue_refilled(int32_t finished, int32_t next, int32_t n) {
  return finished < n - next ? finished : n - next;
}

}  // namespace pb

#endif  // PB_EPISODE_QUEUE_H_
