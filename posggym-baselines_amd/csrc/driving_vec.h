// Driving-v1 step / reward / observation key on the VECTOR ALU.
//
// Same results as the table-driven scalar functions in driving.h (and hence as
// oracle/driving.py); written branch-free with selects so every lane of the
// wave evaluates the identical values in VGPRs.  Why: one CU has one scalar
// ALU shared by its 4 SIMDs but 4 vector ALUs; with every tree's serial logic
// on SALU the scalar unit saturated first.  `vary()` hides the
// wave-uniformity of a value from the compiler so that it stays in a VGPR and
// the arithmetic on it is issued as VALU instead of being scalarised.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "driving.h"

namespace pb {

// (host builds -- the CPU equivalence test against driving.h -- take the identity)
PB_HD uint32_t vary(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t r;
  asm("v_mov_b32 %0, %1" : "=v"(r) : "v"(x));
  return r;
#else
  return x;
#endif
}

struct VPlan {
  uint32_t self, path;
  uint32_t d, speed, cells, done;
};

// The heading and speed changes of action `act` (0..4) come out of two packed
// constants, two bits per action: a chain of conditions on `act` is compiled to
// a divergent branch per action, one issue turn per scalar instruction of it
// (DESIGN.md §4 "Issue slots").
constexpr uint32_t kTurnBits = (1u << (2 * TURN_RIGHT)) | (3u << (2 * TURN_LEFT));   // heading += 1 / 3
constexpr uint32_t kSpeedBits = (1u << (2 * DO_NOTHING)) | (2u << (2 * ACCELERATE)) |   // speed change + 1
                                (0u << (2 * DECELERATE)) | (1u << (2 * TURN_RIGHT)) |
                                (1u << (2 * TURN_LEFT));

PB_HD VPlan vplan(const DrvModel& m, uint32_t self, uint32_t act) {
  VPlan p;
  p.self = self;
  p.done = ((self >> 15) & 3u) != 0u ? 1u : 0u;
  const uint32_t d0 = (self >> 8) & 3u, s0 = (self >> 10) & 3u;
  const uint32_t d = (d0 + ((kTurnBits >> (2u * act)) & 3u)) & 3u;
  const uint32_t t = s0 + ((kSpeedBits >> (2u * act)) & 3u);   // the new speed + 1, unclamped
  const uint32_t sp = (t < 1u ? 1u : (t > 4u ? 4u : t)) - 1u;  // REVERSE .. FORWARD_FAST
  const uint32_t move = (d + (sp != 0u ? 0u : 2u)) & 3u;
  p.d = d;
  p.speed = sp;
  p.cells = sp == 0u ? 1u : sp - 1u;   // |speed - STOPPED|
  p.path = m.nbr2[((self & 0xFFu) << 2) | move];
  return p;
}

struct VMove {
  uint32_t cell, speed, hit;
};

// Cells traversed until a wall or the other vehicle (cell `ocell`).
// (bitwise & and | on the conditions: no short-circuit branches)
PB_HD VMove vresolve(const VPlan& p, uint32_t ocell) {
  const uint32_t c1 = p.path & 0xFFu, c2 = p.path >> 8;
  const uint32_t start = p.self & 0xFFu;
  const bool s1 = p.cells >= 1u;
  const bool w1 = c1 == 0xFFu, h1 = !w1 & (c1 == ocell);
  const bool a1 = s1 & !w1 & !h1;
  const bool s2 = (p.cells >= 2u) & a1;
  const bool w2 = c2 == 0xFFu, h2 = !w2 & (c2 == ocell);
  const bool a2 = s2 & !w2 & !h2;
  VMove r;
  r.cell = a2 ? c2 : (a1 ? c1 : start);
  r.hit = ((s1 & h1) | (s2 & h2)) ? 1u : 0u;
  r.speed = ((s1 & (w1 | h1)) | (s2 & (w2 | h2))) ? (uint32_t)STOPPED : p.speed;
  return r;
}

// The moved vehicle's state; dist = m.g.dist[its destination][mv.cell]
PB_HD uint32_t vfinish(const VPlan& p, const VMove& mv, uint32_t dist) {
  const uint32_t mind0 = (p.self >> 17) & 127u;
  const uint32_t mind = mind0 < dist ? mind0 : dist;
  return (p.self & 0x7F007000u) | mv.cell | (p.d << 8) | (mv.speed << 10) |
         ((dist == 0u ? 1u : 0u) << 15) | (mv.hit << 16) | (mind << 17);
}

// Joint step (drv_step2 semantics).  j: the model-stream draw of the shuffle.
// Both movers' final cells are computed first (a vehicle that does not move
// keeps its own), then both distance reads are issued back to back and
// unconditionally, so that one wait covers them (and the reward's table reads,
// drv_reward_vec); whether a vehicle moved is applied as a select at the end.
PB_HD void drv_step2_vec(const DrvModel& m, uint32_t s0, uint32_t s1, uint32_t a0, uint32_t a1,
                         uint32_t j, uint32_t* o0, uint32_t* o1) {
  const bool first1 = j == 0u;   // shuffle swapped: agent 1 moves first
  const VPlan pf = vplan(m, first1 ? s1 : s0, first1 ? a1 : a0);
  const VPlan ps = vplan(m, first1 ? s0 : s1, first1 ? a0 : a1);
  // first mover against the second's current cell
  const VMove mf = vresolve(pf, ps.self & 0xFFu);
  const bool movef = pf.done == 0u;
  const bool sec_crash = movef & (mf.hit != 0u) & (ps.done == 0u);
  const uint32_t cellf = movef ? mf.cell : (pf.self & 0xFFu);
  // second mover against the first's new cell
  const VMove ms = vresolve(ps, cellf);
  const bool moves = (ps.done == 0u) & !sec_crash;
  const uint32_t cells = moves ? ms.cell : (ps.self & 0xFFu);
  const uint32_t distf = m.g.dist[(pf.self >> 12) & 7u][cellf];
  const uint32_t dists = m.g.dist[(ps.self >> 12) & 7u][cells];
  // (bit merges under an all-ones / all-zeros mask: a select of the whole
  // vfinish value is compiled to a branch around it)
  const uint32_t kf = movef ? ~0u : 0u, ks = moves ? ~0u : 0u;
  uint32_t vf = (vfinish(pf, mf, distf) & kf) | (pf.self & ~kf);
  uint32_t vs = (vfinish(ps, ms, dists) & ks) | (ps.self & ~ks);
  vs |= sec_crash ? (1u << 16) : 0u;
  const bool fst_crash = moves & (ms.hit != 0u) & (((vf >> 15) & 3u) == 0u);
  vf |= fst_crash ? (1u << 16) : 0u;
  *o0 = first1 ? vs : vf;
  *o1 = first1 ? vf : vs;
}

// (the table's rows 1 and 2 are read by `prev` alone, before the step's
// distance reads return; row 0 is 0.0: build_model_tables)
PB_HD double drv_reward_vec(const DrvModel& m, uint32_t prev, uint32_t next) {
  const uint32_t initd = (prev >> 24) & 127u;
  const double p1 = m.prog[128u + initd], p2 = m.prog[256u + initd];
  const bool done0 = ((prev >> 15) & 3u) != 0u;
  const double base = ((next >> 16) & 1u) ? -1.0 : (((next >> 15) & 1u) ? 0.5 : 0.0);
  const uint32_t progress = ((prev >> 17) & 127u) - ((next >> 17) & 127u);   // 0..2
  const double r = base + (progress == 1u ? p1 : (progress == 2u ? p2 : 0.0));
  return done0 ? 0.0 : r;
}

PB_HD int vwindow_index(const DrvGrid& g, int x, int y, int fx, int fy, int rx,
                                             int ry, int tx, int ty) {
  const int dx = tx - x, dy = ty - y;
  const int fwd = dx * fx + dy * fy;
  const int side = dx * rx + dy * ry;
  const bool in = fwd >= -g.obs_back && fwd <= g.obs_front && side >= -g.obs_side &&
                  side <= g.obs_side;
  return in ? (g.obs_front - fwd) * (2 * g.obs_side + 1) + (side + g.obs_side) : -1;
}

PB_HD uint64_t obs_key_vec(const DrvModel& m, uint32_t self, uint32_t other) {
  const DrvGrid& g = m.g;
  const int ncells = (g.obs_front + g.obs_back + 1) * (2 * g.obs_side + 1);
  const uint32_t full = (1u << ncells) - 1u;
  const int x = (int)(self & 15u), y = (int)((self >> 4) & 15u), d = (int)((self >> 8) & 3u);
  const uint32_t wall = m.win_wall[(self & 0xFFu) << 2 | (uint32_t)d];
  uint32_t cells = spread_bits16(wall) | (spread_bits16(~wall & full) << 1);
  const int fx = d == EAST ? 1 : (d == WEST ? -1 : 0);
  const int fy = d == SOUTH ? 1 : (d == NORTH ? -1 : 0);
  const int rx = -fy, ry = fx;   // right of heading d = heading d + 1
  const uint32_t dest = (self >> 12) & 7u;
  const int dxl = g.loc_x[dest], dyl = g.loc_y[dest];
  const int cd = vwindow_index(g, x, y, fx, fy, rx, ry, dxl, dyl);
  const uint32_t dmask = (cd >= 0 && !((wall >> (cd & 31)) & 1u)) ? (3u << (2 * (cd & 15))) : 0u;
  cells |= dmask;
  const int cv = vwindow_index(g, x, y, fx, fy, rx, ry, (int)(other & 15u), (int)((other >> 4) & 15u));
  const uint32_t vmask = (cv >= 0 && !((wall >> (cv & 31)) & 1u)) ? (3u << (2 * (cv & 15))) : 0u;
  cells &= ~vmask;
  const uint64_t tail = ((uint64_t)((self >> 10) & 3u) << 30) | ((uint64_t)x << 32) |
                        ((uint64_t)y << 36) | ((uint64_t)dxl << 40) | ((uint64_t)dyl << 44) |
                        ((uint64_t)((self >> 15) & 1u) << 48) | ((uint64_t)((self >> 16) & 1u) << 49);
  return (uint64_t)cells | tail;
}

}  // namespace pb
