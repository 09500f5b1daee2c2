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

// The tracker's arithmetic on one belief's counts (POMCP.belief_stats,
// planning/pomcp.py; utils.py:292-339): out = {state, policy, action}.
//   n, matches, hist  the counts (hist: kBelAccPolicies bins);
//   num_other         policies the particles carry (0: none -- policy and
//                     action are 0.0);
//   mixture_index     the true policy's bin, -1 (or out of range): not modelled;
//   other_action      the action the other agent just played (< 0: none);
//   other_pi          [num_other][pi_stride] the planner's get_pi tables.
// Python's int / int and int * float on doubles: every integer here is exact
// in a double, each quotient is one correctly rounded division, and the action
// sum adds the non-zero bins' products in ascending order from 0.0 -- with
// contraction off the same roundings as the host's, bit for bit.
constexpr int kBelAccPolicies = 8;
__host__ __device__ inline void bel_accuracy(int32_t n, int32_t matches, const int32_t* hist,
                                             int32_t num_other, int32_t mixture_index,
                                             int32_t other_action, const double* other_pi,
                                             int32_t pi_stride, double out[3]) {
#pragma clang fp contract(off)
  out[0] = out[1] = out[2] = 0.0;
  if (n <= 0) return;
  const double dn = (double)n;
  out[0] = (double)matches / dn;
  if (num_other <= 0) return;
  double pol = 0.0, acc = 0.0;
#pragma unroll
  for (int j = 0; j < kBelAccPolicies; ++j) {
    if (j >= num_other) continue;
    const int32_t h = hist[j];
    if (j == mixture_index) pol = (double)h / dn;
    if (h != 0 && other_action >= 0 && other_action < pi_stride)
      acc = acc + (double)h * other_pi[j * pi_stride + other_action];
  }
  out[1] = pol;
  out[2] = acc / dn;
}

}  // namespace pb

#endif  // PB_BELIEF_STATS_H_
