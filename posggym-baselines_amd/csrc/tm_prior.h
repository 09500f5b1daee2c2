// State-reactive EGO policies of a type-based search: the
// prior line of an obs node, ObsNode.action_probs at its creation, when some
// ego policy of the meta-policy acts on the state instead of drawing from a
// fixed distribution.
//
//   code k + 1  get_pi of ego policy k at the node (potmmcp.py:275-287): its
//               table row when it is fixed, one-hot on its rule's action when
//               it is reactive;
//   code 0      get_expected_action_probs(None, state) (potmmcp.py:391-431):
//               sum_k w_k * pi_k(node) in policy order and action order,
//               divided by its sum accumulated in action order (Python's
//               sum() of a dict's values).  w_k is the normalised expected
//               meta-policy, a constant the caller computed with the
//               reference's own expressions.
//
// Plain C++ with no HIP dependency: k_search and the host twin
// (pomcp_host_tm_prior_line, host_api.cpp) run this one implementation, in
// FP64 without contraction (the build's -ffp-contract=off).
#pragma once
#include <stdint.h>

#include "philox.h"
#include "../../include/pomcp.h"

namespace pb {

constexpr int kTmEgoMax = POMCP_MAX_TYPE_POLICIES;

// The ego policies' kinds (pomcp_set_type_ego_kinds).  Kept beside TmTables,
// not inside it: only the kernels of an environment that has ego kinds stage
// it (k_search<EnvDriving, TM = 1> has no LDS left for it).
struct TmEgo {
  int32_t any;                 // some ego policy is reactive (0: the table path)
  int32_t pad;
  int32_t kind[kTmEgoMax], p0[kTmEgoMax], p1[kTmEgoMax];   // pomcp_policy_kinds
  double w[kTmEgoMax];         // the expected meta-policy, policy order
};

// out[0 .. A) = the prior line of code `code`.  prior: TmTables::prior
// ([code][a]); act(k): reactive ego policy k's action at the node.
template <class Act>
PB_HD void tm_prior_line(const double (*prior)[kTmEgoMax], const TmEgo& e, int n_ego, int A,
                         int code, Act act, double* out) {
  if (code > 0) {
    const int k = code - 1;
    const int ak = e.kind[k] != POMCP_POLICY_FIXED ? (int)act(k) : -1;
#pragma unroll
    for (int a = 0; a < kTmEgoMax; ++a)
      if (a < A) out[a] = ak < 0 ? prior[code][a] : (a == ak ? 1.0 : 0.0);
    return;
  }
  if (!e.any) {
#pragma unroll
    for (int a = 0; a < kTmEgoMax; ++a)
      if (a < A) out[a] = prior[0][a];
    return;
  }
  double acc[kTmEgoMax];
#pragma unroll
  for (int a = 0; a < kTmEgoMax; ++a) acc[a] = 0.0;
  for (int k = 0; k < n_ego; ++k) {
    const int ak = e.kind[k] != POMCP_POLICY_FIXED ? (int)act(k) : -1;
    const double wk = e.w[k];
#pragma unroll
    for (int a = 0; a < kTmEgoMax; ++a)
      if (a < A) acc[a] += wk * (ak < 0 ? prior[k + 1][a] : (a == ak ? 1.0 : 0.0));
  }
  double s = acc[0];   // sum(): 0 + acc[0] is acc[0]
#pragma unroll
  for (int a = 1; a < kTmEgoMax; ++a)
    if (a < A) s = s + acc[a];
#pragma unroll
  for (int a = 0; a < kTmEgoMax; ++a)
    if (a < A) out[a] = acc[a] / s;
}

}  // namespace pb
