// Root-belief statistics (BeliefStatTracker, utils.py:292-339): what one belief
// record {t, v0, v1, aux} contributes to the counts of pomcp_belief_counts
// (include/pomcp.h).  One classification for the device reduction
// (k_belief_stats, belief_stats.hip) and its host twin
// (pomcp_host_belief_counts, host_api.cpp), so the CPU suite and the sanitized
// host build run the code the kernel runs.  Plain C++: no HIP dependency.
#ifndef PB_BELIEF_STATS_H_
#define PB_BELIEF_STATS_H_
#include <stdint.h>

namespace pb {

constexpr uint32_t kBelMatch = 1u;     // v0, v1 equal the query state's (t is not compared:
                                       // get_state_accuracy compares hps.state only)
constexpr uint32_t kBelBadAux = 2u;    // type-based: aux names no other-agent policy
constexpr int kBelPolShift = 8;        // type-based, aux in range: the policy index

// Class word of one record.  has_q = 0: no query state (never a match).
// num_other = 0: a plain context, whose records' aux word is undefined -- it is
// not looked at (pass anything).  An out-of-range aux sets kBelBadAux and
// leaves the policy index 0: the caller must test the flag before it counts.
__host__ __device__ inline uint32_t bel_classify(uint32_t v0, uint32_t v1, uint32_t aux,
                                                 uint32_t q0, uint32_t q1, int has_q,
                                                 uint32_t num_other) {
  uint32_t c = (has_q && v0 == q0 && v1 == q1) ? kBelMatch : 0u;
  if (num_other != 0u) {
    if (aux >= num_other)
      c |= kBelBadAux;
    else
      c |= aux << kBelPolShift;
  }
  return c;
}

}  // namespace pb

#endif  // PB_BELIEF_STATS_H_
