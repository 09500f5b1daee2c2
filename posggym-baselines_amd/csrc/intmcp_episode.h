// One I-NTMCP planner pair's episode, per step: what the step reads of the
// pair (intmcp_episode_root, from its header and root node), which step keeps
// the header's search fields, how a finished pair is parked and how it is
// restored, and what the episode queue's refill does to a slot.  One
// implementation for the device kernels (k_im_episode_step /
// k_im_episode_unpark, intmcp_episode.hip; k_im_queue_refill,
// intmcp_episode_queue.hip) and their host twins (intmcp_host_episode_step /
// intmcp_host_episode_unpark / intmcp_host_episode_refill, host_api.cpp), so the
// CPU suite runs the code the kernels run.  The environment side is
// episode_step.h's episode_step, engine-independent.  Plain C++: no HIP
// dependency.
//
// Parking.  A pair whose episode is over gets INTMCP_SKIP as its next update
// action (k_im_update / k_im_updateN leave it untouched) and the absorbing bit
// of its root node's info word (k_im_search / k_im_searchN run no simulation
// from an absorbing root, allocate nothing and draw nothing; a BEGIN | FINAL
// search still rewrites the header's last_action / num_sims / search_depth
// with 0).  The info word as it was and those three fields go to the pair's
// side record (intmcp_episode_kept) and im_episode_unpark writes them back
// when the batch ends.
#ifndef PB_INTMCP_EPISODE_H_
#define PB_INTMCP_EPISODE_H_
#include <stdint.h>

#include "episode_step.h"
#include "../../include/intmcp.h"

namespace pb {

// INode::info's absorbing bit (intmcp.hip im_absorbing; the device unit asserts
// they agree) and intmcp_update's skip action (kImSkip there).
constexpr uint32_t kImEpAbsorbingBit = 1u << 3;
constexpr int32_t kImEpSkip = INTMCP_SKIP;
// im_episode_step's result for a pair that was finished already: its update
// input stays as it is (INTMCP_SKIP since its last step)
constexpr int32_t kImEpKeepInput = -3;

// The planner's part of the step, at the places k_im_root_stats reads.
PB_HD pomcp_episode_step_in im_episode_step_in(const intmcp_episode_root& r) {
  pomcp_episode_step_in in;
  in.root_absorbing = (r.info & kImEpAbsorbingBit) != 0u ? 1 : 0;
  in.action = r.last_action;
  in.search_depth = r.search_depth;
  in.num_sims = r.num_sims;
  in.error = r.err;
  in.pad = 0;
  in.min_value = r.min_value;
  in.max_value = r.max_value;
  return in;
}

// A real step: the pair was still playing when this step's search ran and the
// search did not fail.  Its header fields are the ones a parked pair shows
// after the batch.  (On an absorbing root the search writes action 0 with no
// simulation at every step, so a pair with an absorbing tail keeps the same
// three values whichever of those steps is counted.)
PB_HD bool im_episode_real(const pomcp_episode_state& before, const pomcp_episode_step_in& in) {
  return before.finished == 0 && in.error == 0;
}

// One step of pair b after its search.  root: in, and out when the pair is
// parked (info gains the absorbing bit: the caller stores it to the root
// node).  Returns the pair's next update action: the ego's action, kImEpSkip
// for a pair that finished in this step (by its episode or by an error) or
// kImEpKeepInput for one that was finished before (nothing changes; out->stepped
// = 0).  *parked = 1 when root->info changed.
template <class E>
PB_HD int32_t im_episode_step(const typename E::Model& m, int ego, intmcp_episode_root* root,
                              intmcp_episode_kept* kept, const double* pow_table, int max_steps,
                              int until, const EpPopTables* pop, int policy_index,
                              pomcp_episode_state* st, pomcp_episode_step_out* out, int* parked) {
  *parked = 0;
  const pomcp_episode_step_in in = im_episode_step_in(*root);
  const bool real = im_episode_real(*st, in);
  const bool was_finished = st->finished != 0;
  episode_step<E>(m, ego, in, pow_table, max_steps, until, pop, policy_index, st, out);
  if (was_finished) return kImEpKeepInput;
  if (real) {
    kept->last_action = root->last_action;
    kept->num_sims = root->num_sims;
    kept->search_depth = root->search_depth;
  }
  if (st->finished == 0) return out->ego_action;
  if (st->res.error == 0 && kept->parked == 0) {
    kept->info = root->info;
    kept->parked = 1;
    root->info |= kImEpAbsorbingBit;
    *parked = 1;
  }
  return kImEpSkip;
}

// The end of the batch for pair b: a parked pair's root info word and header
// fields as its last real step left them.  Returns 1 when root changed; a
// second call finds kept->parked == 0 and changes nothing.
PB_HD int im_episode_unpark(intmcp_episode_root* root, intmcp_episode_kept* kept) {
  if (kept->parked == 0) return 0;
  root->info = kept->info;
  root->last_action = kept->last_action;
  root->num_sims = kept->num_sims;
  root->search_depth = kept->search_depth;
  kept->parked = 0;
  return 1;
}

// The episode queue (intmcp_episodes_queue_begin): what the end of a step does
// to slot b's side record and next update action, given the queue's decision
// for it (episode_queue.h queue_assign).  A new entry (assign >= 0): the slot
// finished in this very step, so im_episode_step has just parked it; the side
// record is cleared with parked = 0 (the unpark at the end of the batch must
// not write the old episode's info word into the new episode's root) and the
// next update is an initial one (action -1).  The absorbing bit the park set
// goes with the node it sits in: the per-pair reset zeroes the pair's node
// blocks and writes a fresh node 0.  Retired (kQueueRetire) or still playing
// (kQueuePlaying): nothing changes, the next action stays as im_episode_step
// left it (kImEpKeepInput).  Returns 1 for a new entry.
PB_HD int im_episode_refill(int32_t assign, intmcp_episode_kept* kept, int32_t* next_action) {
  if (assign < 0) {
    *next_action = kImEpKeepInput;
    return 0;
  }
  kept->info = 0u;
  kept->last_action = -1;
  kept->num_sims = kept->search_depth = 0;
  kept->parked = 0;
  kept->pad[0] = kept->pad[1] = kept->pad[2] = 0;
  *next_action = -1;
  return 1;
}

}  // namespace pb

#endif  // PB_INTMCP_EPISODE_H_
