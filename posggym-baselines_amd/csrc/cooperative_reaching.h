// CooperativeReaching-v0 generative model (host + device), the build's
// restatement (parity with posggym unpinned, the return set
// {0, 0.75, 1.0} pinned by the reference's own
// baseline_exps/env_data/CooperativeReaching-v0 results), and its heuristic
// agents H1-v0 .. H5-v0 (cr_goal_action).
//
// Two agents on an S x S grid (S = 3..8) with a goal in every corner; five
// actions DO_NOTHING, UP (y - 1), DOWN (y + 1), LEFT (x - 1), RIGHT (x + 1); a
// move off the grid leaves the agent in place, the agents do not collide, the
// moves are simultaneous and the step takes no model-stream draw.  When both
// agents stand on the same goal cell after a step, both receive its value and
// both terminate.
//
// State word of an agent:
//   x:3 | y:3 | start x:3 | start y:3 | goal:3
// `goal` is 1 + the index of the goal the agent stands on (0: on none): a
// function of (x, y) every constructor of a word fills in (cr_word), so that
// termination and reward are compares on packed fields of the two words with
// no look-up of the grid (Env::done_of has no model).  The start cell is
// carried so that a heuristic's target is a function of the state.
// Observation key (16 bits): own x:4 | own y:4 | other x:4 | other y:4, the
// other's position (S, S) beyond obs_distance (Chebyshev; < 0: unlimited).
//
// Plain C++ with no HIP dependency: the kernels and the host twins
// (pomcp_cr_*, host_api.cpp) run this one implementation.
#pragma once
#include <stdint.h>

#include "philox.h"
#include "../../include/pomcp.h"

namespace pb {

constexpr int kCrGoals = 4;
constexpr int kCrRules = 5;   // H1 .. H5
constexpr uint32_t kCrPosMask = 0x3Fu;

// Device tables (staged in LDS by every kernel).
struct CrModel {
  int32_t size, obs_distance;       // obs_distance < 0: the other agent is always seen
  uint32_t gcell[kCrGoals];         // (y << 3) | x
  int32_t target[kCrRules][64];     // the goal a heuristic of rule r heads for from start cell c
  double value[8];                  // [0] = 0.0 (on no goal), [k + 1] = goal k's; indexed by the
                                    // 3-bit goal field, so the rest is 0.0 too
};

PB_HD uint32_t cr_x(uint32_t v) { return v & 7u; }
PB_HD uint32_t cr_y(uint32_t v) { return (v >> 3) & 7u; }
PB_HD uint32_t cr_goal_field(uint32_t v) { return (v >> 12) & 7u; }

// 1 + the lowest goal index on cell (y << 3) | x, 0 for none
PB_HD uint32_t cr_goal_of(const CrModel& m, uint32_t cell) {
  uint32_t g = 0u;
  g = cell == m.gcell[3] ? 4u : g;
  g = cell == m.gcell[2] ? 3u : g;
  g = cell == m.gcell[1] ? 2u : g;
  g = cell == m.gcell[0] ? 1u : g;
  return g;
}

// the word of an agent on `cell` that started on `start`
PB_HD uint32_t cr_word(const CrModel& m, uint32_t cell, uint32_t start) {
  return cell | (start << 6) | (cr_goal_of(m, cell) << 12);
}

// The goal a heuristic of `rule` heads for from the start cell (sx, sy):
// Manhattan distance, ties to the lower goal index.
//   0 closest, 1 furthest, 2 closest of value 1.0, 3 furthest of value 1.0,
//   4 closest of value 0.75; a rule no goal qualifies for takes goal 0
template <class G>
inline int cr_rule_target(const G& g, int rule, int sx, int sy) {
  int best = -1, best_d = 0;
  for (int k = 0; k < kCrGoals; ++k) {
    const double val = g.goal_value[k];
    if ((rule == 2 || rule == 3) && val != 1.0) continue;
    if (rule == 4 && val != 0.75) continue;
    const int dx = (int)g.goal[k][0] - sx, dy = (int)g.goal[k][1] - sy;
    const int d = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy);
    const bool far = rule == 1 || rule == 3;
    if (best < 0 || (far ? d > best_d : d < best_d)) {
      best = k;
      best_d = d;
    }
  }
  return best < 0 ? 0 : best;
}

// Host: tables from the description (include/pomcp.h pomcp_cr_grid).
template <class G>
inline void build_cr_model(const G& g, CrModel* m) {
  m->size = g.size;
  m->obs_distance = g.obs_distance;
  for (int k = 0; k < 8; ++k) m->value[k] = 0.0;
  for (int k = 0; k < kCrGoals; ++k) {
    m->gcell[k] = ((uint32_t)(g.goal[k][1] & 7) << 3) | (uint32_t)(g.goal[k][0] & 7);
    m->value[k + 1] = g.goal_value[k];
  }
  for (int r = 0; r < kCrRules; ++r)
    for (int c = 0; c < 64; ++c) m->target[r][c] = cr_rule_target(g, r, c & 7, c >> 3);
}

// false: not the grid this build restates (3..8 cells a side, four goals, one
// in each corner, obs_distance -1 or 0..7)
template <class G>
inline bool cr_grid_ok(const G& g) {
  if (g.size < 3 || g.size > 8 || g.num_goals != kCrGoals) return false;
  if (g.obs_distance < -1 || g.obs_distance > 7) return false;
  uint32_t corners = 0u;
  for (int k = 0; k < kCrGoals; ++k) {
    const int x = g.goal[k][0], y = g.goal[k][1];
    if ((x != 0 && x != g.size - 1) || (y != 0 && y != g.size - 1)) return false;
    corners |= 1u << ((x ? 1 : 0) + (y ? 2 : 0));
    if (!(g.goal_value[k] >= 0.0)) return false;
  }
  return corners == 15u;
}

// One agent's move: branch-free, the coordinate clamped to the grid.
PB_HD uint32_t cr_move(uint32_t v, uint32_t a, int32_t last) {
  const int32_t dx = (int32_t)(a == 4u) - (int32_t)(a == 3u);
  const int32_t dy = (int32_t)(a == 2u) - (int32_t)(a == 1u);
  int32_t x = (int32_t)cr_x(v) + dx, y = (int32_t)cr_y(v) + dy;
  x = x < 0 ? 0 : (x > last ? last : x);
  y = y < 0 ? 0 : (y > last ? last : y);
  return (uint32_t)x | ((uint32_t)y << 3);
}

// Both agents on one goal cell: 1 + its index, else 0.
PB_HD uint32_t cr_joint_goal(uint32_t v0, uint32_t v1) {
  return ((v0 ^ v1) & kCrPosMask) == 0u ? cr_goal_field(v0) : 0u;
}

PB_HD bool cr_done(uint32_t v0, uint32_t v1) { return cr_joint_goal(v0, v1) != 0u; }

// Joint step: the next words and the reward both agents receive.
PB_HD void cr_step(const CrModel& m, uint32_t v0, uint32_t v1, uint32_t a0, uint32_t a1,
                   uint32_t* n0, uint32_t* n1, double* r) {
  const int32_t last = m.size - 1;
  const uint32_t c0 = cr_move(v0, a0, last), c1 = cr_move(v1, a1, last);
  *n0 = c0 | (v0 & 0xFC0u) | (cr_goal_of(m, c0) << 12);
  *n1 = c1 | (v1 & 0xFC0u) | (cr_goal_of(m, c1) << 12);
  *r = m.value[cr_joint_goal(*n0, *n1)];
}

PB_HD uint64_t cr_obs_key(const CrModel& m, int agent, uint32_t v0, uint32_t v1) {
  const uint32_t me = agent == 0 ? v0 : v1, ot = agent == 0 ? v1 : v0;
  const int32_t dx = (int32_t)cr_x(ot) - (int32_t)cr_x(me), dy = (int32_t)cr_y(ot) - (int32_t)cr_y(me);
  const int32_t ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
  const bool hidden = m.obs_distance >= 0 && (ax > ay ? ax : ay) > m.obs_distance;
  const uint32_t ox = hidden ? (uint32_t)m.size : cr_x(ot), oy = hidden ? (uint32_t)m.size : cr_y(ot);
  return (uint64_t)(cr_x(me) | (cr_y(me) << 4) | (ox << 8) | (oy << 12));
}

// The k-th non-goal cell in row-major order (y * S + x), k < S * S - 4.
PB_HD uint32_t cr_free_cell(const CrModel& m, uint32_t k) {
  uint32_t cell = 0u;
  bool found = false;
  for (int32_t y = 0; y < m.size; ++y)
    for (int32_t x = 0; x < m.size; ++x) {
      const uint32_t c = ((uint32_t)y << 3) | (uint32_t)x;
      if (found || cr_goal_of(m, c) != 0u) continue;
      if (k == 0u) {
        cell = c;
        found = true;
      } else {
        --k;
      }
    }
  return cell;
}

// sample_initial_state: agent 0's cell, then agent 1's (model stream).
template <class Draw>
PB_HD void cr_sample_initial_state(const CrModel& m, Draw draw, uint32_t* v0, uint32_t* v1) {
  const uint32_t n = (uint32_t)(m.size * m.size - kCrGoals);
  const uint32_t c0 = cr_free_cell(m, draw(n));
  const uint32_t c1 = cr_free_cell(m, draw(n));
  *v0 = cr_word(m, c0, c0);
  *v1 = cr_word(m, c1, c1);
}

// sample_agent_initial_state: the ego's word from its observation (start =
// position), the other agent's from the observation when it is seen, else
// drawn like an initial cell and rejected until the ego's observation matches
// (<= 64 tries, then the last draw).  false: the observation names a cell
// outside the grid.
template <class Draw>
PB_HD bool cr_sample_agent_initial(const CrModel& m, int agent, uint64_t obs, Draw draw,
                                   uint32_t* v0, uint32_t* v1) {
  const uint32_t S = (uint32_t)m.size;
  const uint32_t x = (uint32_t)(obs & 15u), y = (uint32_t)((obs >> 4) & 15u);
  const uint32_t ox = (uint32_t)((obs >> 8) & 15u), oy = (uint32_t)((obs >> 12) & 15u);
  if (x >= S || y >= S || (obs >> 16) != 0ull) return false;
  const bool seen = ox < S && oy < S;
  if (!seen && !(ox == S && oy == S && m.obs_distance >= 0)) return false;
  const uint32_t ec = x | (y << 3);
  const uint32_t ev = cr_word(m, ec, ec);
  uint32_t ov;
  if (seen) {
    const uint32_t oc = ox | (oy << 3);
    ov = cr_word(m, oc, oc);
  } else {
    const uint32_t n = (uint32_t)(m.size * m.size - kCrGoals);
    ov = 0u;
    for (int tr = 0; tr < 64; ++tr) {
      const uint32_t oc = cr_free_cell(m, draw(n));
      ov = cr_word(m, oc, oc);
      if (cr_obs_key(m, 0, ev, ov) == obs) break;   // (the ego as agent 0 of the pair)
    }
  }
  *v0 = agent == 0 ? ev : ov;
  *v1 = agent == 0 ? ov : ev;
  return true;
}

// The heuristic agent's action (POMCP_POLICY_CR_GOAL, rule 0..4) for the
// agent whose word is `own`: towards its target, horizontally when
// |gx - x| >= |gy - y| and gx != x, else vertically; DO_NOTHING on the target.
PB_HD int cr_goal_action(const CrModel& m, uint32_t own, int rule) {
  const uint32_t gc = m.gcell[m.target[rule][(own >> 6) & 63u]];
  const int32_t dx = (int32_t)(gc & 7u) - (int32_t)cr_x(own);
  const int32_t dy = (int32_t)(gc >> 3) - (int32_t)cr_y(own);
  const int32_t ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
  const int horiz = dx < 0 ? 3 : 4, vert = dy < 0 ? 1 : 2;
  return (ax | ay) == 0 ? 0 : ((ax >= ay && dx != 0) ? horiz : vert);
}

PB_HD bool cr_policy_kind_ok(int kind, int p0, int p1) {
  return kind == POMCP_POLICY_CR_GOAL && p0 >= 0 && p0 < kCrRules && p1 == 0;
}

}  // namespace pb
