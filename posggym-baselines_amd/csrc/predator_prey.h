// PredatorPrey-v0 generative model (host + device), the build's restatement
// (parity with posggym unpinned, the returns 0, 1/3, 2/3, 1 in
// multiples of float32(1/3) and the 50-step limit pinned by the reference's own
// baseline_exps/env_data/PredatorPrey-v0 results).
//
// Two predators (the agents) and 1..3 prey on an open S x S grid (S = 5 or
// 10); five actions DO_NOTHING, UP (y - 1), DOWN (y + 1), LEFT (x - 1),
// RIGHT (x + 1).  One joint step takes ONE model draw j in [0, 2^25): bits
// 0..7, 8..15, 16..23 are the tie bytes of prey 0, 1, 2 and bit 24 is the
// predators' execution order.
//   1. Live prey move in index order, each seeing the moves already made.
//      Candidates: stay (always) and the four moves that stay in the grid and
//      land on no predator and no other live prey.  A predator within
//      Manhattan distance obs_dim (the nearest, ties to the lower index): keep
//      the candidates furthest from it.  Else another live prey within
//      distance 1 (the lowest index): keep those furthest from it.  Else keep
//      all.  The prey takes kept candidate (byte * n) >> 8 in action order.
//   2. The predators move, predator (bit 24) first.  A move off the grid, onto
//      a live prey or onto the other predator's current cell leaves it in place.
//   3. A live prey with >= prey_strength predators at Manhattan distance 1 is
//      caught; both agents receive `reward` = (double)(float)(1.0 / num_prey)
//      per prey caught in the step and both terminate when none is left.
//
// State, two words (cells are 7-bit row-major indices y * S + x):
//   word 0: predator 0:7 | prey 0:7 | prey 1:7 | caught mask:3
//   word 1: predator 1:7 | prey 2:7
// A caught or absent prey has its mask bit set and cell 0, so equal states
// have equal words and done (mask == 7) is a function of the words alone.
// Observation key (<= 49 bits): the (2 * obs_dim + 1)^2 - 1 cells around the
// predator, row-major, two bits each: 0 empty, 1 off the grid, 2 predator,
// 3 live prey; above them one bit: every prey is caught.  No absolute position.
//
// Plain C++ with no HIP dependency: the kernels and the host twins
// (pomcp_pp_*, host_api.cpp) run this one implementation.
#pragma once
#include <stdint.h>

#include "philox.h"
#include "../../include/pomcp.h"

namespace pb {

constexpr int kPpStarts = 8;
constexpr int kPpMaxPrey = 3;
constexpr int kPpMaxBlock = 36;
constexpr uint32_t kPpStepRange = 1u << 25;
constexpr uint32_t kPpCell = 127u;

// Device tables (staged in LDS by every kernel).
struct PpModel {
  int32_t size, num_prey, strength, obs_dim;
  uint32_t recip;                    // ceil(65536 / size): y = (cell * recip) >> 16
  int32_t n_block;                   // cells of the prey's start block
  uint32_t absent;                   // the caught-mask bits of the prey there are not
  uint32_t pad;
  uint32_t start[kPpStarts];         // the predators' start cells, row-major
  uint32_t block[kPpMaxBlock];       // the prey's start cells, row-major
  uint64_t start_pat[kPpStarts];     // the off-grid cells of the observation on start[k]
  double reward;                     // per prey caught
};

// The unpacked state the rules work on.
struct PpState {
  int32_t px[2], py[2], qx[kPpMaxPrey], qy[kPpMaxPrey];
  uint32_t caught;
};

PB_HD int32_t pp_abs(int32_t v) { return v < 0 ? -v : v; }
PB_HD int32_t pp_dx(int a) { return (int32_t)(a == 4) - (int32_t)(a == 3); }
PB_HD int32_t pp_dy(int a) { return (int32_t)(a == 2) - (int32_t)(a == 1); }

PB_HD void pp_xy(const PpModel& m, uint32_t cell, int32_t* x, int32_t* y) {
  const uint32_t yy = (cell * m.recip) >> 16;
  *y = (int32_t)yy;
  *x = (int32_t)(cell - yy * (uint32_t)m.size);
}
PB_HD uint32_t pp_cell(const PpModel& m, int32_t x, int32_t y) {
  return (uint32_t)(y * m.size + x);
}

PB_HD void pp_unpack(const PpModel& m, uint32_t w0, uint32_t w1, PpState* s) {
  pp_xy(m, w0 & kPpCell, &s->px[0], &s->py[0]);
  pp_xy(m, w1 & kPpCell, &s->px[1], &s->py[1]);
  pp_xy(m, (w0 >> 7) & kPpCell, &s->qx[0], &s->qy[0]);
  pp_xy(m, (w0 >> 14) & kPpCell, &s->qx[1], &s->qy[1]);
  pp_xy(m, (w1 >> 7) & kPpCell, &s->qx[2], &s->qy[2]);
  s->caught = (w0 >> 21) & 7u;
}

// (a caught prey's cell is 0)
PB_HD void pp_pack(const PpModel& m, const PpState& s, uint32_t* w0, uint32_t* w1) {
  uint32_t q[kPpMaxPrey];
#pragma unroll
  for (int k = 0; k < kPpMaxPrey; ++k)
    q[k] = ((s.caught >> k) & 1u) ? 0u : pp_cell(m, s.qx[k], s.qy[k]);
  *w0 = pp_cell(m, s.px[0], s.py[0]) | (q[0] << 7) | (q[1] << 14) | (s.caught << 21);
  *w1 = pp_cell(m, s.px[1], s.py[1]) | (q[2] << 7);
}

PB_HD bool pp_done(uint32_t w0) { return ((w0 >> 21) & 7u) == 7u; }

// a live prey other than `skip` stands on (x, y)
PB_HD bool pp_prey_on(const PpState& s, int skip, int32_t x, int32_t y) {
  bool on = false;
#pragma unroll
  for (int i = 0; i < kPpMaxPrey; ++i)
    on = on || (i != skip && !((s.caught >> i) & 1u) && s.qx[i] == x && s.qy[i] == y);
  return on;
}

// Prey k's move (rule 1 of the header): straight-line, candidates as a 5-bit
// mask, the choice by popcount and k-th set bit.  *rule: 0 a predator, 1 a
// prey, 2 neither decided it (for the tests; dead code elsewhere).
PB_HD void pp_move_prey(const PpModel& m, PpState* s, int k, uint32_t byte, int* rule) {
  const int32_t S = m.size, x = s->qx[k], y = s->qy[k];
  const int32_t d0 = pp_abs(x - s->px[0]) + pp_abs(y - s->py[0]);
  const int32_t d1 = pp_abs(x - s->px[1]) + pp_abs(y - s->py[1]);
  const bool near0 = d0 <= m.obs_dim, near1 = d1 <= m.obs_dim;
  const bool from_pred = near0 || near1;
  const bool second = near1 && (!near0 || d1 < d0);   // ties to the lower index
  int32_t tx = second ? s->px[1] : s->px[0], ty = second ? s->py[1] : s->py[0];
  bool from_prey = false;
  int32_t ux = 0, uy = 0;
#pragma unroll
  for (int i = kPpMaxPrey - 1; i >= 0; --i) {   // (descending: the lowest index stays)
    const bool nb = i != k && !((s->caught >> i) & 1u) &&
                    pp_abs(x - s->qx[i]) + pp_abs(y - s->qy[i]) <= 1;
    from_prey = from_prey || nb;
    ux = nb ? s->qx[i] : ux;
    uy = nb ? s->qy[i] : uy;
  }
  tx = from_pred ? tx : ux;
  ty = from_pred ? ty : uy;
  const bool flee = from_pred || from_prey;
  *rule = from_pred ? 0 : (from_prey ? 1 : 2);
  uint32_t cand = 0u;
  int32_t dist[5], best = -1;
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    const int32_t nx = x + pp_dx(a), ny = y + pp_dy(a);
    const bool ok = a == 0 || (nx >= 0 && nx < S && ny >= 0 && ny < S &&
                               !(nx == s->px[0] && ny == s->py[0]) &&
                               !(nx == s->px[1] && ny == s->py[1]) && !pp_prey_on(*s, k, nx, ny));
    dist[a] = flee ? pp_abs(nx - tx) + pp_abs(ny - ty) : 0;
    best = (ok && dist[a] > best) ? dist[a] : best;
    cand |= (ok ? 1u : 0u) << a;
  }
  uint32_t keep = 0u;
#pragma unroll
  for (int a = 0; a < 5; ++a) keep |= ((((cand >> a) & 1u) != 0u && dist[a] == best) ? 1u : 0u) << a;
  const uint32_t idx = (byte * (uint32_t)__builtin_popcount(keep)) >> 8;
  uint32_t cnt = 0u;
  int sel = 0;
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    const uint32_t bit = (keep >> a) & 1u;
    sel = (bit != 0u && cnt == idx) ? a : sel;
    cnt += bit;
  }
  const bool live = !((s->caught >> k) & 1u);
  s->qx[k] = live ? x + pp_dx(sel) : x;
  s->qy[k] = live ? y + pp_dy(sel) : y;
}

// A predator on (*x, *y) moves by `a` with the other predator on (ox, oy);
// *blocked: a move (a != 0) that left it in place.
PB_HD void pp_move_predator(const PpModel& m, const PpState& s, int32_t* x, int32_t* y, uint32_t a,
                            int32_t ox, int32_t oy, bool* blocked) {
  const int32_t S = m.size;
  const int32_t nx = *x + pp_dx((int)a), ny = *y + pp_dy((int)a);
  const bool ok = nx >= 0 && nx < S && ny >= 0 && ny < S && !(nx == ox && ny == oy) &&
                  !pp_prey_on(s, -1, nx, ny);
  *blocked = a != 0u && !ok;
  *x = ok ? nx : *x;
  *y = ok ? ny : *y;
}

// What a step did beside the next state (the generator's conditions).
struct PpStepInfo {
  int rule[kPpMaxPrey];   // the rule that decided prey k's move, -1: not live
  int blocked[2];         // predator i moved and was held in place
};

// Joint step: the next words and the number of prey caught.
PB_HD void pp_step_info(const PpModel& m, uint32_t w0, uint32_t w1, uint32_t a0, uint32_t a1,
                        uint32_t j, uint32_t* n0, uint32_t* n1, uint32_t* ncaught,
                        PpStepInfo* info) {
  PpState s;
  pp_unpack(m, w0, w1, &s);
#pragma unroll
  for (int k = 0; k < kPpMaxPrey; ++k) {
    int rule;
    pp_move_prey(m, &s, k, (j >> (8 * k)) & 255u, &rule);
    info->rule[k] = ((s.caught >> k) & 1u) ? -1 : rule;
  }
  const bool swap = ((j >> 24) & 1u) != 0u;
  // (branch-free: the first mover and the second by selects on the order bit)
  int32_t fx = swap ? s.px[1] : s.px[0], fy = swap ? s.py[1] : s.py[0];
  int32_t gx = swap ? s.px[0] : s.px[1], gy = swap ? s.py[0] : s.py[1];
  bool fb, gb;
  pp_move_predator(m, s, &fx, &fy, swap ? a1 : a0, gx, gy, &fb);
  pp_move_predator(m, s, &gx, &gy, swap ? a0 : a1, fx, fy, &gb);
  s.px[0] = swap ? gx : fx;
  s.py[0] = swap ? gy : fy;
  s.px[1] = swap ? fx : gx;
  s.py[1] = swap ? fy : gy;
  const bool b0 = swap ? gb : fb, b1 = swap ? fb : gb;
  info->blocked[0] = b0 ? 1 : 0;
  info->blocked[1] = b1 ? 1 : 0;
  uint32_t n = 0u;
#pragma unroll
  for (int k = 0; k < kPpMaxPrey; ++k) {
    const int32_t e0 = pp_abs(s.qx[k] - s.px[0]) + pp_abs(s.qy[k] - s.py[0]);
    const int32_t e1 = pp_abs(s.qx[k] - s.px[1]) + pp_abs(s.qy[k] - s.py[1]);
    const bool hit = !((s.caught >> k) & 1u) &&
                     (int32_t)(e0 == 1) + (int32_t)(e1 == 1) >= m.strength;
    n += hit ? 1u : 0u;
    s.caught |= (hit ? 1u : 0u) << k;
  }
  pp_pack(m, s, n0, n1);
  *ncaught = n;
}

PB_HD void pp_step(const PpModel& m, uint32_t w0, uint32_t w1, uint32_t a0, uint32_t a1, uint32_t j,
                   uint32_t* n0, uint32_t* n1, double* r) {
  uint32_t n;
  PpStepInfo info;
  pp_step_info(m, w0, w1, a0, a1, j, n0, n1, &n, &info);
  *r = (double)n * m.reward;
}

// The off-grid cells (code 1) of the W x W window around (x, y), centre
// included, W = 2 * obs_dim + 1, two bits a cell, row-major.
PB_HD uint64_t pp_offgrid(const PpModel& m, int32_t x, int32_t y) {
  const int32_t d = m.obs_dim, W = 2 * d + 1, last = m.size - 1;
  const int32_t lx = d - x > 0 ? d - x : 0, hx = d - (last - x) > 0 ? d - (last - x) : 0;
  const int32_t ly = d - y > 0 ? d - y : 0, hy = d - (last - y) > 0 ? d - (last - y) : 0;
  const uint32_t rowfull = 0x155u & ((1u << (2 * W)) - 1u);
  const uint32_t colpat = rowfull & (((1u << (2 * lx)) - 1u) | ~((1u << (2 * (W - hx))) - 1u));
  uint64_t full = 0ull;
#pragma unroll
  for (int r = 0; r < 5; ++r) {
    const bool off = r < ly || r >= W - hy;
    const uint64_t row = (uint64_t)(off ? rowfull : colpat) << (2 * W * (r < W ? r : 0));
    full |= r < W ? row : 0ull;
  }
  return full;
}

PB_HD uint64_t pp_obs_key(const PpModel& m, int agent, uint32_t w0, uint32_t w1) {
  PpState s;
  pp_unpack(m, w0, w1, &s);
  const int32_t d = m.obs_dim, W = 2 * d + 1;
  const int32_t mx = agent == 0 ? s.px[0] : s.px[1], my = agent == 0 ? s.py[0] : s.py[1];
  const int32_t ox = agent == 0 ? s.px[1] : s.px[0], oy = agent == 0 ? s.py[1] : s.py[0];
  uint64_t full = pp_offgrid(m, mx, my);
  {
    const uint32_t rx = (uint32_t)(ox - mx + d), ry = (uint32_t)(oy - my + d);
    const bool in = rx < (uint32_t)W && ry < (uint32_t)W;
    full |= in ? 2ull << (2u * (ry * (uint32_t)W + rx)) : 0ull;
  }
#pragma unroll
  for (int k = 0; k < kPpMaxPrey; ++k) {
    const uint32_t rx = (uint32_t)(s.qx[k] - mx + d), ry = (uint32_t)(s.qy[k] - my + d);
    const bool in = !((s.caught >> k) & 1u) && rx < (uint32_t)W && ry < (uint32_t)W;
    full |= in ? 3ull << (2u * (ry * (uint32_t)W + rx)) : 0ull;
  }
  // the centre cell (the predator itself) is not part of the key; the bit above
  // the window says that no prey is left (the step's terminal flag, which the
  // planners receive beside the observation: an observation child has ONE
  // absorbing flag, so a terminal step must not share its key with another)
  const uint32_t c = 2u * (uint32_t)(2 * d * (d + 1));
  const uint64_t over = (uint64_t)(s.caught == 7u ? 1u : 0u) << (2 * (W * W - 1));
  return (full & ((1ull << c) - 1ull)) | ((full >> (c + 2u)) << c) | over;
}

// The prey in turn: a cell of the start block that no earlier prey took.
template <class Draw>
PB_HD void pp_draw_prey(const PpModel& m, Draw& draw, uint32_t q[kPpMaxPrey]) {
  for (int k = 0; k < kPpMaxPrey; ++k) q[k] = 0u;
  for (int k = 0; k < m.num_prey; ++k) {
    uint32_t i = draw((uint32_t)(m.n_block - k));
    uint32_t cell = 0u;
    bool found = false;
    for (int b = 0; b < m.n_block; ++b) {
      const uint32_t c = m.block[b];
      bool taken = false;
      for (int e = 0; e < k; ++e) taken = taken || q[e] == c;
      if (found || taken) continue;
      if (i == 0u) {
        cell = c;
        found = true;
      } else {
        --i;
      }
    }
    q[k] = cell;
  }
}

PB_HD void pp_words(const PpModel& m, uint32_t p0, uint32_t p1, const uint32_t q[kPpMaxPrey],
                    uint32_t* w0, uint32_t* w1) {
  *w0 = p0 | (q[0] << 7) | (q[1] << 14) | (m.absent << 21);
  *w1 = p1 | (q[2] << 7);
}

// sample_initial_state: predator 0's start cell, predator 1's among the other
// seven, then the prey (model stream; every choice over the cells still free
// in row-major order).
template <class Draw>
PB_HD void pp_sample_initial_state(const PpModel& m, Draw draw, uint32_t* w0, uint32_t* w1) {
  const uint32_t i0 = draw((uint32_t)kPpStarts);
  uint32_t i1 = draw((uint32_t)kPpStarts - 1u);
  i1 += i1 >= i0 ? 1u : 0u;
  uint32_t q[kPpMaxPrey];
  pp_draw_prey(m, draw, q);
  pp_words(m, m.start[i0], m.start[i1], q, w0, w1);
}

// sample_agent_initial_state: the agent stands on the start cell whose
// off-grid pattern is the observation's (false: none); the other predator and
// the prey are drawn as the initial state draws them and rejected until the
// whole observation matches (<= 64 tries, then the last draw).
template <class Draw>
PB_HD bool pp_sample_agent_initial(const PpModel& m, int agent, uint64_t obs, Draw draw,
                                   uint32_t* w0, uint32_t* w1) {
  const int32_t W = 2 * m.obs_dim + 1;
  if ((obs >> (2 * (W * W - 1))) != 0ull) return false;
  const uint64_t lo = 0x5555555555555555ull;
  const uint64_t pat = obs & lo & ~((obs >> 1) & lo);
  int si = -1;
  for (int k = kPpStarts - 1; k >= 0; --k) si = m.start_pat[k] == pat ? k : si;
  if (si < 0) return false;
  const uint32_t ec = m.start[si];
  for (int tr = 0; tr < 64; ++tr) {
    uint32_t i = draw((uint32_t)kPpStarts - 1u);
    i += i >= (uint32_t)si ? 1u : 0u;
    const uint32_t oc = m.start[i];
    uint32_t q[kPpMaxPrey];
    pp_draw_prey(m, draw, q);
    pp_words(m, agent == 0 ? ec : oc, agent == 0 ? oc : ec, q, w0, w1);
    if (pp_obs_key(m, agent, *w0, *w1) == obs) break;
  }
  return true;
}

// The start cells of an S x S grid in row-major order: the corners and the
// edge cells at x or y = S / 2.
inline void pp_start_cells(int size, uint8_t out[kPpStarts][2]) {
  const int l = size - 1, h = size / 2;
  const int xy[kPpStarts][2] = {{0, 0}, {h, 0}, {l, 0}, {0, h}, {l, h}, {0, l}, {h, l}, {l, l}};
  for (int k = 0; k < kPpStarts; ++k) {
    out[k][0] = (uint8_t)xy[k][0];
    out[k][1] = (uint8_t)xy[k][1];
  }
}

PB_HD double pp_capture_reward(int num_prey) { return (double)(float)(1.0 / (double)num_prey); }

// false: not a grid this build restates ("5x5" or "10x10", open; 1..3 prey,
// prey_strength 1..2, obs_dim 1..2, the start cells and the reward the rules give)
template <class G>
inline bool pp_grid_ok(const G& g) {
  if (g.size != 5 && g.size != 10) return false;
  if (g.num_prey < 1 || g.num_prey > kPpMaxPrey) return false;
  if (g.prey_strength < 1 || g.prey_strength > 2) return false;
  if (g.obs_dim < 1 || g.obs_dim > 2) return false;
  uint8_t want[kPpStarts][2];
  pp_start_cells(g.size, want);
  for (int k = 0; k < kPpStarts; ++k)
    if (g.start[k][0] != want[k][0] || g.start[k][1] != want[k][1]) return false;
  return g.capture_reward == pp_capture_reward(g.num_prey);
}

// Host: tables from the description (include/pomcp.h pomcp_pp_grid).
template <class G>
inline void build_pp_model(const G& g, PpModel* m) {
  m->size = g.size;
  m->num_prey = g.num_prey;
  m->strength = g.prey_strength;
  m->obs_dim = g.obs_dim;
  m->recip = (65536u + (uint32_t)g.size - 1u) / (uint32_t)g.size;
  m->absent = 7u & ~((1u << g.num_prey) - 1u);
  m->pad = 0u;
  m->reward = g.capture_reward;
  // the prey's start block: the central (S - 4) x (S - 4) cells; S = 5: the
  // centre and its 4-neighbours
  m->n_block = 0;
  for (int k = 0; k < kPpMaxBlock; ++k) m->block[k] = 0u;
  const int c = g.size / 2;
  for (int y = 0; y < g.size; ++y)
    for (int x = 0; x < g.size; ++x) {
      const bool in = g.size == 5 ? pp_abs(x - c) + pp_abs(y - c) <= 1
                                  : (x >= 2 && x < g.size - 2 && y >= 2 && y < g.size - 2);
      if (in && m->n_block < kPpMaxBlock) m->block[m->n_block++] = pp_cell(*m, x, y);
    }
  for (int k = 0; k < kPpStarts; ++k) {
    m->start[k] = pp_cell(*m, g.start[k][0], g.start[k][1]);
    const uint64_t full = pp_offgrid(*m, g.start[k][0], g.start[k][1]);
    const uint32_t cb = 2u * (uint32_t)(2 * g.obs_dim * (g.obs_dim + 1));
    m->start_pat[k] = (full & ((1ull << cb) - 1ull)) | ((full >> (cb + 2u)) << cb);
  }
}

// false: words that are no state of the model (a cell off the grid, two
// entities on one cell, a caught prey with a cell, set bits beyond the fields)
inline bool pp_state_ok(const PpModel& m, const uint32_t state[2]) {
  const uint32_t w0 = state[0], w1 = state[1];
  if ((w0 >> 24) != 0u || (w1 >> 14) != 0u) return false;
  const uint32_t caught = (w0 >> 21) & 7u;
  if ((caught & m.absent) != m.absent) return false;
  const uint32_t cells[5] = {w0 & kPpCell, w1 & kPpCell, (w0 >> 7) & kPpCell, (w0 >> 14) & kPpCell,
                             (w1 >> 7) & kPpCell};
  const uint32_t n = (uint32_t)(m.size * m.size);
  for (int i = 0; i < 5; ++i) {
    const bool live = i < 2 || !((caught >> (i - 2)) & 1u);
    if (!live) {
      if (cells[i] != 0u) return false;
      continue;
    }
    if (cells[i] >= n) return false;
    for (int k = 0; k < i; ++k) {
      const bool lk = k < 2 || !((caught >> (k - 2)) & 1u);
      if (lk && cells[k] == cells[i]) return false;
    }
  }
  return true;
}

}  // namespace pb
