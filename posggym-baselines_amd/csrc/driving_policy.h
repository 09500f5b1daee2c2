// State-reactive other-agent policies of Driving-v1 (host + device): the
// shortest-path agents Driving-v1/A{0,40,60,80,100}Shortestpath-v0 of the
// reference's Driving experiments (baseline_exps/env_data/Driving-v1/
// agents_P0.yaml), the build's restatement (DESIGN.md §20 "State-reactive
// other-agent policies"; planning/policies.py ShortestPathPolicy is the same rule on
// observations).
//
// A Driving observation is a function of the state and the heading changes
// only with the agent's own turns, so the action is a pure function of the two
// packed vehicle words (driving.h) and two integers:
//   caution  rows of the observation window ahead in which another vehicle
//            makes the agent brake (0: it never brakes for traffic)
//   vmax     the speed it does not exceed while another choice exists
// The episode kernels play it for a population member (episode_step.h) and the
// type-based search for a particle's modelled policy (k_search<TM = 1>,
// k_update).  One implementation for the kernels and the host twin
// (pomcp_host_driving_policy_actions), plain C++ with no HIP dependency.
//
// Bounds: x, y are 4-bit fields and the tables have a 16-wide stride, so a
// vehicle's own cell always indexes inside wall[256] / dist[8][256]; a
// neighbouring cell (x + dx = -1 or 16 at a border start cell, the front cell
// of a vehicle at its destination) is looked up only after grid_free has
// placed it inside the grid.
#pragma once
#include <stdint.h>

#include "driving.h"
#include "../../include/pomcp.h"

namespace pb {

// Another vehicle in the first min(caution, obs_front) rows ahead, at most
// obs_side cells aside, in the agent's heading frame: the VEHICLE cells of
// those rows of its observation (a vehicle is never on a wall cell and nothing
// occludes).
template <class G>
PB_HD bool drv_sp_threat(const G& g, uint32_t own, uint32_t other, int caution) {
  const int d = (own >> 8) & 3, r = (d + 1) & 3;
  const int rx = (int)(other & 15) - (int)(own & 15);
  const int ry = (int)((other >> 4) & 15) - (int)((own >> 4) & 15);
  const int fwd = rx * dir_dx(d) + ry * dir_dy(d);
  const int side = rx * dir_dx(r) + ry * dir_dy(r);
  const int rows = caution < g.obs_front ? caution : g.obs_front;
  return fwd >= 1 && fwd <= rows && side >= -g.obs_side && side <= g.obs_side;
}

// The shortest-path agent's action for the vehicle `own` beside `other`.
template <class G>
PB_HD int drv_sp_action(const G& g, uint32_t own, uint32_t other, int caution, int vmax) {
  if (veh_done(own)) return DO_NOTHING;
  const int speed = (own >> 10) & 3;
  if (drv_sp_threat(g, own, other, caution))
    return speed > STOPPED ? DECELERATE : (speed < STOPPED ? ACCELERATE : DO_NOTHING);
  const int dest = (own >> 12) & 7;
  int best = 0;
  uint32_t best_key = 0xFFFFFFFFu;
  for (int a = 0; a < 5; ++a) {   // action order; the first minimum wins
    int d = (own >> 8) & 3, sp = speed;
    if (a == TURN_RIGHT) d = (d + 1) & 3;
    else if (a == TURN_LEFT) d = (d + 3) & 3;
    else if (a == ACCELERATE) sp = sp + 1 < FORWARD_FAST ? sp + 1 : FORWARD_FAST;
    else if (a == DECELERATE) sp = sp - 1 > REVERSE ? sp - 1 : REVERSE;
    const uint32_t over = sp > vmax ? 1u : 0u;
    const int move = sp != REVERSE ? d : ((d + 2) & 3);
    const int cells = sp > STOPPED ? sp - STOPPED : STOPPED - sp;
    int x = own & 15, y = (own >> 4) & 15;
    uint32_t bumped = 0u;
    // the model's move on the static grid, vehicles ignored
    for (int k = 0; k < cells; ++k) {
      const int nx = x + dir_dx(move), ny = y + dir_dy(move);
      if (!grid_free(g, nx, ny)) {
        bumped = 1u;
        break;
      }
      x = nx;
      y = ny;
    }
    const uint32_t dist = g.dist[dest][(y << 4) | x];
    const int fx = x + dir_dx(d), fy = y + dir_dy(d);
    const uint32_t ahead =
        dist == 0u ? 0u : (grid_free(g, fx, fy) ? (uint32_t)g.dist[dest][(fy << 4) | fx] : 127u);
    // (over, bumped, dist, ahead) in lexicographic order: a distance is a BFS
    // length (< 127 on a 16 x 16 grid) or 127 for an unreachable cell, as is
    // `ahead` behind a wall, so each fits its 8 bits
    const uint32_t key = (over << 17) | (bumped << 16) | (dist << 8) | ahead;
    if (key < best_key) {
      best = a;
      best_key = key;
    }
  }
  return best;
}

// kind / parameters of one policy of a population or a mixture
// (pomcp_policy_kinds): false for an unknown kind or a parameter out of range.
PB_HD bool drv_policy_kind_ok(int kind, int p0, int p1) {
  if (kind == POMCP_POLICY_FIXED) return true;
  return kind == POMCP_POLICY_DRIVING_SHORTEST_PATH && p0 >= 0 && p0 <= 15 && p1 >= REVERSE &&
         p1 <= FORWARD_FAST;
}

}  // namespace pb
