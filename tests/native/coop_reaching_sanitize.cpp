// Stand-alone walk of csrc/cooperative_reaching.h under the sanitizers
// (tests/test_coop_reaching_host.py compiles it with g++ -fsanitize=address,
// undefined and runs it; no Python-loaded code is involved).
//
// For size 3, 5 and 8 and obs_distance -1 (always seen) and 1: every pair of
// agent cells x every pair of start cells on the diagonal x every joint
// action goes through cr_step, both observation keys and every rule of
// cr_goal_action, the border cells -- where x - 1 / y + 1 leave the grid --
// included; every observation a state gives goes through
// cr_sample_agent_initial for both agents.  The next words are checked against
// a plain restatement.  Prints the number of steps and a checksum; exits 0
// when no sanitizer stopped it and every check held.
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../posggym-baselines_amd/csrc/cooperative_reaching.h"

static pomcp_cr_grid make_grid(int size, int obs_distance) {
  pomcp_cr_grid g{};
  g.size = size;
  g.obs_distance = obs_distance;
  g.num_goals = 4;
  const int s = size - 1;
  const int cells[4][2] = {{0, 0}, {s, s}, {0, s}, {s, 0}};
  const double values[4] = {1.0, 1.0, 0.75, 0.75};
  for (int k = 0; k < 4; ++k) {
    g.goal[k][0] = (uint8_t)cells[k][0];
    g.goal[k][1] = (uint8_t)cells[k][1];
    g.goal_value[k] = values[k];
  }
  return g;
}

static void fail(const char* what, int size, uint32_t v0, uint32_t v1, int a0, int a1) {
  std::fprintf(stderr, "%s: size %d words %u %u actions %d %d\n", what, size, v0, v1, a0, a1);
  std::exit(2);
}

int main() {
  long long steps = 0, sum = 0;
  const int sizes[3] = {3, 5, 8}, dists[2] = {-1, 1};
  for (int size : sizes)
    for (int od : dists) {
      const pomcp_cr_grid g = make_grid(size, od);
      if (!pb::cr_grid_ok(g)) return 3;
      pb::CrModel* m = new pb::CrModel;   // on the heap: a read past its end is a report
      pb::build_cr_model(g, m);
      const int n = size * size;
      uint32_t ctr = 12345u;
      auto draw = [&](uint32_t k) {
        ctr = ctr * 1664525u + 1013904223u;
        return (uint32_t)(((uint64_t)ctr * k) >> 32);
      };
      for (int c0 = 0; c0 < n; ++c0)
        for (int c1 = 0; c1 < n; ++c1)
          for (int st = 0; st < n; ++st) {
            const uint32_t p0 = (uint32_t)(c0 % size) | ((uint32_t)(c0 / size) << 3);
            const uint32_t p1 = (uint32_t)(c1 % size) | ((uint32_t)(c1 / size) << 3);
            const uint32_t s0 = (uint32_t)(st % size) | ((uint32_t)(st / size) << 3);
            const uint32_t s1 = (uint32_t)((n - 1 - st) % size) | ((uint32_t)((n - 1 - st) / size) << 3);
            const uint32_t v0 = pb::cr_word(*m, p0, s0), v1 = pb::cr_word(*m, p1, s1);
            for (int i = 0; i < 2; ++i) {
              const uint64_t key = pb::cr_obs_key(*m, i, v0, v1);
              uint32_t q0, q1;
              if (!pb::cr_sample_agent_initial(*m, i, key, draw, &q0, &q1))
                fail("sample_agent_initial refused a model observation", size, v0, v1, -1, -1);
              if (((i == 0 ? q0 : q1) & pb::kCrPosMask) != ((i == 0 ? v0 : v1) & pb::kCrPosMask))
                fail("sample_agent_initial moved the ego", size, v0, v1, -1, -1);
              sum += (long long)key + q0 + q1;
              for (int rule = 0; rule < pb::kCrRules; ++rule) {
                const int a = pb::cr_goal_action(*m, i == 0 ? v0 : v1, rule);
                if (a < 0 || a > 4) fail("rule action out of range", size, v0, v1, rule, a);
                sum += a;
              }
            }
            for (int a0 = 0; a0 < 5; ++a0)
              for (int a1 = 0; a1 < 5; ++a1) {
                uint32_t n0, n1;
                double r;
                pb::cr_step(*m, v0, v1, (uint32_t)a0, (uint32_t)a1, &n0, &n1, &r);
                ++steps;
                // the plain restatement
                const int dx[5] = {0, 0, 0, -1, 1}, dy[5] = {0, -1, 1, 0, 0};
                int x0 = c0 % size + dx[a0], y0 = c0 / size + dy[a0];
                int x1 = c1 % size + dx[a1], y1 = c1 / size + dy[a1];
                if (x0 < 0 || x0 >= size) x0 = c0 % size;
                if (y0 < 0 || y0 >= size) y0 = c0 / size;
                if (x1 < 0 || x1 >= size) x1 = c1 % size;
                if (y1 < 0 || y1 >= size) y1 = c1 / size;
                if ((int)pb::cr_x(n0) != x0 || (int)pb::cr_y(n0) != y0 || (int)pb::cr_x(n1) != x1 ||
                    (int)pb::cr_y(n1) != y1 || ((n0 >> 6) & 63u) != s0 || ((n1 >> 6) & 63u) != s1)
                  fail("step moved wrongly", size, v0, v1, a0, a1);
                double want = 0.0;
                for (int k = 3; k >= 0; --k)
                  if (x0 == x1 && y0 == y1 && x0 == g.goal[k][0] && y0 == g.goal[k][1])
                    want = g.goal_value[k];
                if (r != want || pb::cr_done(n0, n1) != (want != 0.0))
                  fail("reward / termination", size, v0, v1, a0, a1);
                sum += (long long)pb::cr_obs_key(*m, 0, n0, n1) + (long long)pb::cr_obs_key(*m, 1, n0, n1) +
                       (long long)(r * 4.0);
              }
          }
      delete m;
    }
  std::printf("%lld %lld\n", steps, sum);
  return 0;
}
