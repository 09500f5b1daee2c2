// The PredatorPrey-v0 heuristic agents H1 .. H3 (POMCP_POLICY_PP_HEURISTIC,
// param0 = rule 0..2, param1 = 0), the build's restatement (DESIGN.md §24;
// planning/policies.py PreyHeuristicPolicy is the same rule in Python).
//
// Unlike the Driving and CooperativeReaching agents these are STOCHASTIC
// reactive policies: the rule gives a distribution over up to four moves that
// depends on the state, and the word of the agent's action stream picks from
// it as random.choices(range(5), weights=pi) does.
//
// For the predator on (x, y) with the other predator on (ox, oy), D = obs_dim:
//   seen      a cell within Chebyshev distance D (the observation window);
//   near      the seen live prey of least Manhattan distance, ties by the
//             window's row-major order (smaller dy, then smaller dx);
//   rule 0    target = near, else the other predator if seen, else none;
//   rule 1    target = the other predator if seen and further than 1, else near;
//   rule 2    with a seen prey and the other predator seen: the seen prey of
//             least distance to the other predator (ties: distance to the agent,
//             then window order); else as rule 0;
//   free(a)   the cell after move a is on the grid, holds no live prey and is
//             not (ox, oy);
//   no target: the free moves; a target: the free moves that bring the agent
//   closer to it (at most two); none: DO_NOTHING.  pi is uniform over these.
// Everything read lies inside the agent's observation window, so the rule is a
// function of the last observation as well as of the two state words.
//
// Plain C++ with no HIP dependency: the kernels and the host twins
// (pomcp_host_pp_policy_*, host_api.cpp) run this one implementation.
#pragma once
#include <stdint.h>

#include "philox.h"
#include "predator_prey.h"
#include "../../include/pomcp.h"

namespace pb {

constexpr int kPpRules = 3;
constexpr int32_t kPpNoKey = 0x7fffffff;

PB_HD bool pp_policy_kind_ok(int kind, int p0, int p1) {
  return kind == POMCP_POLICY_PP_HEURISTIC && p0 >= 0 && p0 < kPpRules && p1 == 0;
}

// The moves 1..4 the rule is uniform over, bit a - 1 for move a (0: DO_NOTHING
// alone).  Straight-line: the target by a packed key, the candidates a mask.
PB_HD uint32_t pp_heuristic_mask(const PpModel& m, int agent, uint32_t w0, uint32_t w1, int rule) {
  PpState s;
  pp_unpack(m, w0, w1, &s);
  const int32_t S = m.size, D = m.obs_dim;
  const int32_t x = agent == 0 ? s.px[0] : s.px[1], y = agent == 0 ? s.py[0] : s.py[1];
  const int32_t ox = agent == 0 ? s.px[1] : s.px[0], oy = agent == 0 ? s.py[1] : s.py[0];
  const int32_t mdx = pp_abs(ox - x), mdy = pp_abs(oy - y);
  const bool mate = mdx <= D && mdy <= D;
  const int32_t mate_d = mdx + mdy;
  // near: key (distance, dy, dx); by_mate: (distance to the other predator, key)
  int32_t nkey = kPpNoKey, nx_ = 0, ny_ = 0, mkey = kPpNoKey, mx_ = 0, my_ = 0;
#pragma unroll
  for (int k = 0; k < kPpMaxPrey; ++k) {
    const int32_t dx = s.qx[k] - x, dy = s.qy[k] - y;
    const bool in = !((s.caught >> k) & 1u) && pp_abs(dx) <= D && pp_abs(dy) <= D;
    const int32_t key = ((pp_abs(dx) + pp_abs(dy)) * 5 + (dy + 2)) * 5 + (dx + 2);   // < 128
    const int32_t k1 = in ? key : kPpNoKey;
    const int32_t k2 = in ? ((pp_abs(s.qx[k] - ox) + pp_abs(s.qy[k] - oy)) << 7) + key : kPpNoKey;
    const bool b1 = k1 < nkey, b2 = k2 < mkey;
    nkey = b1 ? k1 : nkey;
    nx_ = b1 ? s.qx[k] : nx_;
    ny_ = b1 ? s.qy[k] : ny_;
    mkey = b2 ? k2 : mkey;
    mx_ = b2 ? s.qx[k] : mx_;
    my_ = b2 ? s.qy[k] : my_;
  }
  const bool any = nkey != kPpNoKey;
  // rule 0 (and rule 2 without both in sight): near, else the mate
  bool has = any || mate;
  int32_t tx = any ? nx_ : ox, ty = any ? ny_ : oy;
  const bool r1 = rule == 1, r1m = mate && mate_d > 1, r2 = rule == 2 && any && mate;
  has = r1 ? (r1m || any) : has;
  tx = r1 ? (r1m ? ox : nx_) : (r2 ? mx_ : tx);
  ty = r1 ? (r1m ? oy : ny_) : (r2 ? my_ : ty);
  const int32_t here = pp_abs(tx - x) + pp_abs(ty - y);
  uint32_t cand = 0u;
#pragma unroll
  for (int a = 1; a < 5; ++a) {
    const int32_t cx = x + pp_dx(a), cy = y + pp_dy(a);
    const bool fr = cx >= 0 && cx < S && cy >= 0 && cy < S && !(cx == ox && cy == oy) &&
                    !pp_prey_on(s, -1, cx, cy);
    const bool closer = pp_abs(tx - cx) + pp_abs(ty - cy) < here;
    cand |= ((fr && (!has || closer)) ? 1u : 0u) << (a - 1);
  }
  return cand;
}

// random.choices' cumulative weights of the rule's pi, by the additions
// itertools.accumulate makes in action order; 1.0 / n is a constant the host
// compiler rounds, not a device division.
PB_HD void pp_heuristic_cum(const PpModel& m, int agent, uint32_t w0, uint32_t w1, int rule,
                            double cum[5]) {
  const uint32_t cand = pp_heuristic_mask(m, agent, w0, w1, rule);
  const int n = __builtin_popcount(cand);
  const double p = n == 1 ? 1.0 : (n == 2 ? 0.5 : (n == 3 ? 1.0 / 3.0 : 0.25));
  double acc = n == 0 ? 1.0 : 0.0;
  cum[0] = acc;
#pragma unroll
  for (int a = 1; a < 5; ++a) {
    acc = acc + (((cand >> (a - 1)) & 1u) ? p : 0.0);
    cum[a] = acc;
  }
}

// The rule's pi itself (the host twin's output).
PB_HD void pp_heuristic_pi(const PpModel& m, int agent, uint32_t w0, uint32_t w1, int rule,
                           double pi[5]) {
  const uint32_t cand = pp_heuristic_mask(m, agent, w0, w1, rule);
  const int n = __builtin_popcount(cand);
  const double p = n == 1 ? 1.0 : (n == 2 ? 0.5 : (n == 3 ? 1.0 / 3.0 : 0.25));
  pi[0] = n == 0 ? 1.0 : 0.0;
#pragma unroll
  for (int a = 1; a < 5; ++a) pi[a] = ((cand >> (a - 1)) & 1u) ? p : 0.0;
}

// sample_action: bisect_right(cum, random() * (cum[4] + 0.0), 0, 4) on `word`
// (ep_choice / tm_choice on the row the rule built).
PB_HD int pp_heuristic_action(const PpModel& m, int agent, uint32_t w0, uint32_t w1, int rule,
                              uint32_t word) {
  double cum[5];
  pp_heuristic_cum(m, agent, w0, w1, rule, cum);
  const double x = uniform_float(word) * (cum[4] + 0.0);
  int i = 4;
#pragma unroll
  for (int q = 3; q >= 0; --q) i = x < cum[q] ? q : i;
  return i;
}

}  // namespace pb
