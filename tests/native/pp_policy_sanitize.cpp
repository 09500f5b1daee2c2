// Stand-alone walk of csrc/predator_prey_policy.h under the sanitizers
// (tests/test_predator_prey_agents_host.py compiles it with g++
// -fsanitize=address,undefined and runs it; no Python-loaded code is involved).
//
// Every state of the 5x5 grid with one prey (two predators on distinct cells,
// the prey on a third or caught: 25 * 24 * 24) and 20,000 sampled states of the
// 10x10 grid with three prey, caught ones among them, go through the rule for
// both agents and every rule: the mask of moves, its cumulative weights, the
// distribution and the draw on eight words.  A plain restatement of the
// candidate test checks the mask's moves (on the grid, off every live prey and
// the other predator), the weights must end at the sum the distribution has,
// and every drawn action must have positive probability.  The host twins
// pomcp_host_pp_policy_* (one translation unit with them) serve the same
// states through heap arrays of the exact size, and refuse what they must.
// Prints the two state counts and a checksum; exits 0 when no sanitizer
// stopped it and every check held.
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

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

static void fail(const char* what, uint32_t w0, uint32_t w1, int agent, int rule) {
  std::fprintf(stderr, "%s: words %u %u agent %d rule %d\n", what, w0, w1, agent, rule);
  std::exit(2);
}

static long long check_state(const pb::PpModel& m, uint32_t w0, uint32_t w1, uint32_t salt) {
  long long sum = 0;
  const uint32_t st[2] = {w0, w1};
  if (!pb::pp_state_ok(m, st)) fail("not a state", w0, w1, -1, -1);
  pb::PpState s;
  pb::pp_unpack(m, w0, w1, &s);
  for (int agent = 0; agent < 2; ++agent)
    for (int rule = 0; rule < pb::kPpRules; ++rule) {
      const uint32_t mask = pb::pp_heuristic_mask(m, agent, w0, w1, rule);
      if (mask > 15u) fail("mask out of range", w0, w1, agent, rule);
      const int dx[5] = {0, 0, 0, -1, 1}, dy[5] = {0, -1, 1, 0, 0};
      for (int a = 1; a < 5; ++a) {
        if (!((mask >> (a - 1)) & 1u)) continue;
        const int x = s.px[agent] + dx[a], y = s.py[agent] + dy[a];
        bool ok = x >= 0 && x < m.size && y >= 0 && y < m.size &&
                  !(x == s.px[1 - agent] && y == s.py[1 - agent]);
        for (int k = 0; k < pb::kPpMaxPrey; ++k)
          if (!((s.caught >> k) & 1u) && s.qx[k] == x && s.qy[k] == y) ok = false;
        if (!ok) fail("a move that is not free", w0, w1, agent, rule);
      }
      double* cum = new double[5];   // on the heap: a write past its end is a report
      double* pi = new double[5];
      pb::pp_heuristic_cum(m, agent, w0, w1, rule, cum);
      pb::pp_heuristic_pi(m, agent, w0, w1, rule, pi);
      double acc = pi[0];
      for (int a = 1; a < 5; ++a) acc = acc + pi[a];
      if (cum[4] != acc || !(cum[4] > 0.99) || !(cum[4] < 1.01))
        fail("cumulative weights", w0, w1, agent, rule);
      for (uint32_t i = 0; i < 8u; ++i) {
        const uint32_t word = i == 0u ? 0u : (i == 1u ? 0xffffffffu : (salt + i) * 2654435761u);
        const int a = pb::pp_heuristic_action(m, agent, w0, w1, rule, word);
        if (a < 0 || a > 4 || !(pi[a] > 0.0)) fail("an action outside the support", w0, w1, agent, rule);
        sum += a;
      }
      sum += (long long)mask;
      delete[] cum;
      delete[] pi;
    }
  return sum;
}

// the host twins on exactly-sized heap arrays
static long long twins(const pomcp_pp_grid& g, const std::vector<uint32_t>& w0,
                       const std::vector<uint32_t>& w1) {
  const int64_t n = (int64_t)w0.size();
  long long sum = 0;
  for (int agent = 0; agent < 2; ++agent)
    for (int rule = 0; rule < pb::kPpRules; ++rule) {
      double* pi = new double[(size_t)n * 5];
      int32_t* act = new int32_t[(size_t)n];
      uint32_t* words = new uint32_t[(size_t)n];
      for (int64_t i = 0; i < n; ++i) words[i] = (uint32_t)i * 2246822519u + 0x9e3779b9u;
      if (pomcp_host_pp_policy_pi(&g, n, w0.data(), w1.data(), agent, rule, pi) != POMCP_OK ||
          pomcp_host_pp_policy_actions(&g, n, w0.data(), w1.data(), agent, rule, words, act) !=
              POMCP_OK)
        fail("a twin refused", 0u, 0u, agent, rule);
      for (int64_t i = 0; i < n; ++i) {
        if (act[i] < 0 || act[i] > 4 || !(pi[i * 5 + act[i]] > 0.0))
          fail("twin action outside the support", w0[(size_t)i], w1[(size_t)i], agent, rule);
        sum += act[i];
      }
      delete[] pi;
      delete[] act;
      delete[] words;
    }
  double one[5];
  int32_t a1[1];
  const uint32_t z[1] = {w0[0]}, z1[1] = {w1[0]}, wd[1] = {1u};
  if (pomcp_host_pp_policy_pi(nullptr, 1, z, z1, 0, 0, one) != POMCP_E_INVALID ||
      pomcp_host_pp_policy_pi(&g, -1, z, z1, 0, 0, one) != POMCP_E_INVALID ||
      pomcp_host_pp_policy_pi(&g, 1, nullptr, z1, 0, 0, one) != POMCP_E_INVALID ||
      pomcp_host_pp_policy_pi(&g, 1, z, z1, 2, 0, one) != POMCP_E_INVALID ||
      pomcp_host_pp_policy_pi(&g, 1, z, z1, 0, 3, one) != POMCP_E_INVALID ||
      pomcp_host_pp_policy_pi(&g, 1, z, z1, 0, -1, one) != POMCP_E_INVALID ||
      pomcp_host_pp_policy_actions(&g, 1, z, z1, 0, 3, wd, a1) != POMCP_E_INVALID ||
      pomcp_host_pp_policy_actions(&g, 1, z, z1, 0, 0, nullptr, a1) != POMCP_E_INVALID ||
      pomcp_host_pp_policy_actions(&g, 1, z, z1, 0, 0, wd, nullptr) != POMCP_E_INVALID ||
      pomcp_host_pp_policy_actions(&g, 0, nullptr, nullptr, 0, 0, nullptr, nullptr) != POMCP_OK)
    fail("a twin's refusals", 0u, 0u, -1, -1);
  return sum;
}

int main() {
  long long states = 0, sampled = 0, sum = 0;
  {
    const pomcp_pp_grid g = make_grid(5, 1, 1, 1);
    if (!pb::pp_grid_ok(g)) return 3;
    pb::PpModel* m = new pb::PpModel;   // on the heap: a read past its end is a report
    pb::build_pp_model(g, m);
    std::vector<uint32_t> w0s, w1s;
    for (uint32_t c0 = 0; c0 < 25u; ++c0)
      for (uint32_t c1 = 0; c1 < 25u; ++c1) {
        if (c1 == c0) continue;
        for (int q = -1; q < 25; ++q) {
          if (q == (int)c0 || q == (int)c1) continue;
          const uint32_t caught = q < 0 ? 7u : 6u;
          const uint32_t w0 = c0 | ((q < 0 ? 0u : (uint32_t)q) << 7) | (caught << 21), w1 = c1;
          sum += check_state(*m, w0, w1, (uint32_t)states);
          w0s.push_back(w0);
          w1s.push_back(w1);
          ++states;
        }
      }
    sum += twins(g, w0s, w1s);
    delete m;
  }
  {
    const pomcp_pp_grid g = make_grid(10, 3, 2, 2);
    if (!pb::pp_grid_ok(g)) return 3;
    pb::PpModel* m = new pb::PpModel;
    pb::build_pp_model(g, m);
    uint32_t ctr = 2463534242u;
    auto draw = [&](uint32_t k) {
      ctr = ctr * 1664525u + 1013904223u;
      return (uint32_t)(((uint64_t)ctr * k) >> 32);
    };
    std::vector<uint32_t> w0s, w1s;
    while (sampled < 20000) {
      uint32_t c[5];
      bool distinct = true;
      for (int i = 0; i < 5; ++i) {
        c[i] = draw(100u);
        for (int k = 0; k < i; ++k) distinct = distinct && c[k] != c[i];
      }
      if (!distinct) continue;
      const uint32_t caught = draw(8u);
      for (int k = 0; k < 3; ++k)
        if ((caught >> k) & 1u) c[2 + k] = 0u;
      const uint32_t w0 = c[0] | (c[2] << 7) | (c[3] << 14) | (caught << 21);
      const uint32_t w1 = c[1] | (c[4] << 7);
      sum += check_state(*m, w0, w1, (uint32_t)sampled);
      w0s.push_back(w0);
      w1s.push_back(w1);
      ++sampled;
    }
    sum += twins(g, w0s, w1s);
    delete m;
  }
  std::printf("%lld %lld %lld\n", states, sampled, sum);
  return 0;
}
