// Stand-alone walk of csrc/tm_prior.h (the prior line of a node under
// state-reactive ego policies) under the sanitizers
// (tests/test_reactive_ego_host.py compiles it with g++ -fsanitize=address,
// undefined and runs it; no Python-loaded code is involved).
//
// On the grids of size 3 and 8, every 6-bit cell and start cell of the packed
// word -- cells outside the smaller grid included -- goes through every prior
// code for 1 and 8 ego policies with every mix of fixed and reactive kinds the
// low bits of a counter select.  A line must be a distribution (code 0) or
// one-hot / the table row (code k + 1).  Prints the number of lines and of bad
// ones; exits 0 when no sanitizer stopped it.
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../../posggym-baselines_amd/csrc/cooperative_reaching.h"
#include "../../posggym-baselines_amd/csrc/tm_prior.h"

int main() {
  long long calls = 0, bad = 0;
  const int A = 5;
  for (int size : {3, 8}) {
    pomcp_cr_grid g{};
    g.size = size;
    g.obs_distance = -1;
    g.num_goals = 4;
    const int s = size - 1;
    const int corner[4][2] = {{0, 0}, {s, s}, {0, s}, {s, 0}};
    const double val[4] = {1.0, 1.0, 0.75, 0.75};
    for (int k = 0; k < 4; ++k) {
      g.goal[k][0] = corner[k][0];
      g.goal[k][1] = corner[k][1];
      g.goal_value[k] = val[k];
    }
    if (!pb::cr_grid_ok(g)) return 2;
    pb::CrModel* m = new pb::CrModel;   // on the heap: a read past its end is a report
    pb::build_cr_model(g, m);
    for (int n_ego : {1, pb::kTmEgoMax}) {
      // heap tables of exactly the rows in use
      auto* prior = new double[n_ego + 1][pb::kTmEgoMax];
      for (int c = 0; c <= n_ego; ++c)
        for (int a = 0; a < pb::kTmEgoMax; ++a) prior[c][a] = a < A ? (a == c % A ? 0.6 : 0.1) : 0.0;
      for (uint32_t mix = 0; mix < 4; ++mix) {
        pb::TmEgo* e = new pb::TmEgo{};
        for (int k = 0; k < n_ego; ++k) {
          const bool reactive = ((mix >> (k & 1)) & 1u) != 0u;
          e->kind[k] = reactive ? POMCP_POLICY_CR_GOAL : POMCP_POLICY_FIXED;
          e->p0[k] = k % pb::kCrRules;
          e->w[k] = 1.0 / n_ego;
          e->any |= reactive ? 1 : 0;
        }
        for (uint32_t cell = 0; cell < 64; ++cell)
          for (uint32_t start = 0; start < 64; ++start) {
            const uint32_t own = cell | (start << 6);
            for (int code = 0; code <= n_ego; ++code) {
              double out[A];
              pb::tm_prior_line(prior, *e, n_ego, A, code,
                                [&](int k) { return pb::cr_goal_action(*m, own, e->p0[k]); }, out);
              double sum = 0.0;
              int ones = 0;
              for (int a = 0; a < A; ++a) {
                if (!(out[a] >= 0.0 && out[a] <= 1.0)) ++bad;
                sum += out[a];
                ones += out[a] == 1.0;
              }
              if (std::fabs(sum - 1.0) > 1e-12) ++bad;
              if (code > 0 && e->kind[code - 1] != POMCP_POLICY_FIXED && ones != 1) ++bad;
              if (code > 0 && e->kind[code - 1] == POMCP_POLICY_FIXED && out[code % A] != 0.6) ++bad;
              ++calls;
            }
          }
        delete e;
      }
      delete[] prior;
    }
    delete m;
  }
  std::printf("%lld %lld\n", calls, bad);
  return bad == 0 ? 0 : 3;
}
