// Stand-alone walk of csrc/predator_prey.h under the sanitizers
// (tests/test_predator_prey_host.py compiles it with g++ -fsanitize=address,
// undefined and runs it; no Python-loaded code is involved).
//
// The hand-built states of that test (a capture by two predators and none by
// one at strength 2, one by one at strength 1, two prey in one step, a predator
// blocked by the edge, a prey and the other predator in both orders, a cornered
// prey) and, on each of the 24 accepted descriptions, 200 walks of 50 random
// joint steps from sampled initial states go through pp_step_info, both
// observation keys and pp_sample_agent_initial -- the code the kernels run --
// and the host twins pomcp_pp_* of host_api.cpp run episodes of their own with
// their refusals (host_twins).  Every next state must be a state of the
// model (pp_state_ok), every key within its window's bits.  Prints the number
// of walk steps, the captures and a checksum; exits 0 when no sanitizer stopped
// it and every check held.
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#include <cstdint>
#include <cstdio>
#include <cstdlib>

// (one translation unit with the host twins: host_api.cpp is plain C++)
#include "../../posggym-baselines_amd/csrc/host_api.cpp"

static pomcp_pp_grid make_grid(int size, int num_prey, int strength, int obs_dim) {
  pomcp_pp_grid g{};
  g.size = size;
  g.num_prey = num_prey;
  g.prey_strength = strength;
  g.obs_dim = obs_dim;
  pb::pp_start_cells(size, g.start);
  g.capture_reward = pb::pp_capture_reward(num_prey);
  return g;
}

static void fail(const char* what, uint32_t w0, uint32_t w1, int a0, int a1, uint32_t j) {
  std::fprintf(stderr, "%s: words %u %u actions %d %d draw %u\n", what, w0, w1, a0, a1, j);
  std::exit(2);
}

struct Cell {
  int x, y;
};

// words of predators p0, p1 and the live prey q[0 .. n) on m's grid
static void words(const pb::PpModel& m, Cell p0, Cell p1, const Cell* q, int n, uint32_t* w0,
                  uint32_t* w1) {
  uint32_t c[pb::kPpMaxPrey] = {0u, 0u, 0u};
  uint32_t caught = 7u;
  for (int k = 0; k < n; ++k) {
    c[k] = pb::pp_cell(m, q[k].x, q[k].y);
    caught &= ~(1u << k);
  }
  *w0 = pb::pp_cell(m, p0.x, p0.y) | (c[0] << 7) | (c[1] << 14) | (caught << 21);
  *w1 = pb::pp_cell(m, p1.x, p1.y) | (c[2] << 7);
}

struct Out {
  uint32_t n0, n1, caught;
  pb::PpStepInfo info;
};

static Out step(const pb::PpModel& m, uint32_t w0, uint32_t w1, int a0, int a1, uint32_t j) {
  Out o;
  const uint32_t in[2] = {w0, w1};
  if (!pb::pp_state_ok(m, in)) fail("not a state before the step", w0, w1, a0, a1, j);
  pb::pp_step_info(m, w0, w1, (uint32_t)a0, (uint32_t)a1, j, &o.n0, &o.n1, &o.caught, &o.info);
  const uint32_t out[2] = {o.n0, o.n1};
  if (!pb::pp_state_ok(m, out)) fail("not a state after the step", w0, w1, a0, a1, j);
  return o;
}

static void hand_built() {
  pb::PpModel* m = new pb::PpModel;   // on the heap: a read past its end is a report
  uint32_t w0, w1;
  {   // a prey that stays (no predator within obs_dim 1, tie byte 0): two predators catch it
      // at strength 2, one does not
    pb::build_pp_model(make_grid(5, 1, 2, 1), m);
    const Cell q[1] = {{0, 0}};
    words(*m, {0, 2}, {2, 0}, q, 1, &w0, &w1);
    Out o = step(*m, w0, w1, 1, 3, 0u);
    if (o.caught != 1u || !pb::pp_done(o.n0)) fail("two predators", w0, w1, 1, 3, 0u);
    o = step(*m, w0, w1, 1, 0, 0u);
    if (o.caught != 0u || pb::pp_done(o.n0)) fail("one predator at strength 2", w0, w1, 1, 0, 0u);
    pb::build_pp_model(make_grid(5, 1, 1, 1), m);
    o = step(*m, w0, w1, 1, 0, 0u);
    if (o.caught != 1u || !pb::pp_done(o.n0)) fail("one predator at strength 1", w0, w1, 1, 0, 0u);
  }
  {   // two prey in one step
    pb::build_pp_model(make_grid(10, 3, 1, 1), m);
    const Cell q[3] = {{0, 0}, {9, 0}, {5, 9}};
    words(*m, {0, 2}, {9, 2}, q, 3, &w0, &w1);
    const Out o = step(*m, w0, w1, 1, 1, 0u);
    if (o.caught != 2u || ((o.n0 >> 21) & 7u) != 3u) fail("two prey", w0, w1, 1, 1, 0u);
  }
  {   // blocked by the edge, a prey, the other predator, in both orders
    pb::build_pp_model(make_grid(10, 1, 2, 1), m);
    for (uint32_t order = 0; order < 2; ++order) {
      const uint32_t j = order << 24;
      const Cell far[1] = {{5, 5}}, corner[1] = {{0, 0}};
      words(*m, {0, 0}, {9, 9}, far, 1, &w0, &w1);
      Out o = step(*m, w0, w1, 3, 4, j);
      if (o.info.blocked[0] != 1 || o.info.blocked[1] != 1 || o.n0 != w0 || o.n1 != w1)
        fail("the edge", w0, w1, 3, 4, j);
      words(*m, {1, 0}, {0, 1}, corner, 1, &w0, &w1);   // (the prey has no way out: it stays)
      o = step(*m, w0, w1, 3, 0, j);
      if (o.info.blocked[0] != 1 || (o.n0 & pb::kPpCell) != 1u) fail("a prey", w0, w1, 3, 0, j);
    }
    const Cell far[1] = {{8, 8}};
    words(*m, {3, 3}, {4, 3}, far, 1, &w0, &w1);
    Out o = step(*m, w0, w1, 4, 4, 0u);
    if (o.info.blocked[0] != 1 || (o.n0 & pb::kPpCell) != 33u) fail("the other predator", w0, w1, 4, 4, 0u);
    o = step(*m, w0, w1, 4, 4, 1u << 24);
    if (o.info.blocked[0] != 0 || (o.n0 & pb::kPpCell) != 34u) fail("the freed cell", w0, w1, 4, 4, 1u << 24);
  }
  {   // a cornered prey has the single candidate stay, whatever its byte
    pb::build_pp_model(make_grid(5, 2, 2, 1), m);
    const Cell q[2] = {{0, 0}, {0, 1}};
    words(*m, {1, 0}, {4, 4}, q, 2, &w0, &w1);
    for (uint32_t byte = 0; byte < 256u; ++byte) {
      const Out o = step(*m, w0, w1, 0, 0, byte);
      if (((o.n0 >> 7) & pb::kPpCell) != 0u || ((o.n0 >> 21) & 1u) != 0u)
        fail("the cornered prey moved", w0, w1, 0, 0, byte);
    }
  }
  delete m;
}

// The host twins themselves (host_api.cpp pomcp_pp_*): their argument checks,
// pp_state_ok and the model counter's write-back, on every description.
static long long host_twins() {
  long long sum = 0;
  const int sizes[2] = {5, 10};
  for (int size : sizes)
    for (int np = 1; np <= 3; ++np)
      for (int strength = 1; strength <= 2; ++strength)
        for (int od = 1; od <= 2; ++od) {
          const pomcp_pp_grid g = make_grid(size, np, strength, od);
          for (uint64_t seed = 0; seed < 20; ++seed) {
            uint32_t ctr = 0u, st[2], nx[2];
            if (pomcp_pp_sample_initial_state(&g, seed, 7u, &ctr, st) != POMCP_OK ||
                ctr != 2u + (uint32_t)np)
              fail("twin: sample_initial_state", st[0], st[1], -1, -1, ctr);
            uint64_t keys[2];
            if (pomcp_pp_obs(&g, st, keys) != POMCP_OK) fail("twin: obs", st[0], st[1], -1, -1, 0u);
            for (int i = 0; i < 2; ++i) {
              uint32_t c2 = ctr, q[2];
              if (pomcp_pp_sample_agent_initial_state(&g, i, keys[i], seed, 7u, &c2, q) != POMCP_OK ||
                  (c2 - ctr) % (1u + (uint32_t)np) != 0u || c2 == ctr)
                fail("twin: sample_agent_initial_state", st[0], st[1], i, -1, c2);
              if (pomcp_pp_sample_agent_initial_state(&g, i, keys[i] | (1ull << 62), seed, 7u, &c2,
                                                      q) != POMCP_E_INVALID)
                fail("twin: took bits beyond the window", st[0], st[1], i, -1, c2);
              sum += q[0] + q[1];
            }
            for (int t = 0; t < 50; ++t) {
              const int32_t act[2] = {(int32_t)((seed + 3 * t) % 5), (int32_t)((seed * 7 + t * t) % 5)};
              double rew[2];
              int32_t term[2];
              const uint32_t before = ctr;
              if (pomcp_pp_step(&g, st, act, seed, 7u, &ctr, nx, rew, term, keys) != POMCP_OK ||
                  ctr != before + 1u || rew[0] != rew[1] || term[0] != term[1])
                fail("twin: step", st[0], st[1], act[0], act[1], ctr);
              sum += nx[0] + nx[1] + (long long)(keys[0] & 0xFFFFull);
              if (term[0]) break;
              st[0] = nx[0];
              st[1] = nx[1];
            }
            // refused: a bad action, words that are no state, a null pointer; the counter stays
            const int32_t bad_act[2] = {5, 0}, ok_act[2] = {0, 0};
            double rew[2];
            int32_t term[2];
            const uint32_t before = ctr;
            const uint32_t no_state[2] = {st[0] | (1u << 24), st[1]};
            if (pomcp_pp_step(&g, st, bad_act, seed, 7u, &ctr, nx, rew, term, keys) != POMCP_E_INVALID ||
                pomcp_pp_step(&g, no_state, ok_act, seed, 7u, &ctr, nx, rew, term, keys) != POMCP_E_INVALID ||
                pomcp_pp_step(&g, st, ok_act, seed, 7u, nullptr, nx, rew, term, keys) != POMCP_E_INVALID ||
                pomcp_pp_obs(&g, no_state, keys) != POMCP_E_INVALID || ctr != before)
              fail("twin: refusals", st[0], st[1], -1, -1, ctr);
          }
          pomcp_pp_grid bad = g;
          bad.num_prey = 4;
          uint32_t ctr = 0u, st[2];
          if (pomcp_pp_sample_initial_state(&bad, 0, 0u, &ctr, st) != POMCP_E_INVALID)
            fail("twin: took a bad description", 0u, 0u, -1, -1, 0u);
        }
  return sum;
}

int main() {
  hand_built();
  if (host_twins() <= 0) return 4;
  long long steps = 0, captures = 0, sum = 0;
  const int sizes[2] = {5, 10};
  for (int size : sizes)
    for (int np = 1; np <= 3; ++np)
      for (int strength = 1; strength <= 2; ++strength)
        for (int od = 1; od <= 2; ++od) {
          const pomcp_pp_grid g = make_grid(size, np, strength, od);
          if (!pb::pp_grid_ok(g)) return 3;
          pb::PpModel* m = new pb::PpModel;
          pb::build_pp_model(g, m);
          uint32_t ctr = 12345u + (uint32_t)(size * 64 + np * 16 + strength * 4 + od);
          auto draw = [&](uint32_t k) {
            ctr = ctr * 1664525u + 1013904223u;
            return (uint32_t)(((uint64_t)ctr * k) >> 32);
          };
          const int W = 2 * od + 1;
          const uint64_t key_bits = (1ull << (2 * (W * W - 1) + 1)) - 1ull;   // cells + the no-prey-left bit
          for (int walk = 0; walk < 200; ++walk) {
            uint32_t w0, w1;
            pb::pp_sample_initial_state(*m, draw, &w0, &w1);
            for (int i = 0; i < 2; ++i) {
              const uint64_t key = pb::pp_obs_key(*m, i, w0, w1);
              uint32_t q0, q1;
              if (!pb::pp_sample_agent_initial(*m, i, key, draw, &q0, &q1))
                fail("sample_agent_initial refused an initial observation", w0, w1, i, -1, 0u);
              if (((i == 0 ? q0 : q1) & pb::kPpCell) != ((i == 0 ? w0 : w1) & pb::kPpCell))
                fail("sample_agent_initial moved the agent", w0, w1, i, -1, 0u);
              const uint32_t q[2] = {q0, q1};
              if (!pb::pp_state_ok(*m, q)) fail("sample_agent_initial: not a state", q0, q1, i, -1, 0u);
              // a lone off-grid cell in the middle of the window is no start cell's pattern
              if (pb::pp_sample_agent_initial(*m, i, 1ull << (2 * ((W * W - 1) / 2)), draw, &q0, &q1))
                fail("sample_agent_initial took an inconsistent observation", w0, w1, i, -1, 0u);
              sum += (long long)(key & 0xFFFFFFull) + q0 + q1;
            }
            for (int t = 0; t < 50; ++t) {
              if (pb::pp_done(w0)) pb::pp_sample_initial_state(*m, draw, &w0, &w1);
              const int a0 = (int)draw(5u), a1 = (int)draw(5u);
              const uint32_t j = draw(pb::kPpStepRange);
              const Out o = step(*m, w0, w1, a0, a1, j);
              ++steps;
              captures += o.caught;
              for (int i = 0; i < 2; ++i) {
                const uint64_t key = pb::pp_obs_key(*m, i, o.n0, o.n1);
                if ((key & ~key_bits) != 0ull) fail("key beyond its window", o.n0, o.n1, a0, a1, j);
                sum += (long long)(key & 0xFFFFFFull);
              }
              double r;
              uint32_t r0, r1;
              pb::pp_step(*m, w0, w1, (uint32_t)a0, (uint32_t)a1, j, &r0, &r1, &r);
              if (r0 != o.n0 || r1 != o.n1 || r != (double)o.caught * g.capture_reward)
                fail("pp_step differs from pp_step_info", w0, w1, a0, a1, j);
              w0 = o.n0;
              w1 = o.n1;
              sum += w0 + w1;
            }
          }
          delete m;
        }
  std::printf("%lld %lld %lld\n", steps, captures, sum);
  return 0;
}
