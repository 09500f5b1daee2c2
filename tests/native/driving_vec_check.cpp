// Host build of csrc/driving_vec.h (the Driving-v1 step, reward and
// observation key as k_search computes them) against the scalar functions of
// csrc/driving.h, case by case (tests/test_driving_vec_host.py).
//
//   driving_vec_check FILE     FILE = a DrvGrid, then N x {s0, s1, a0, a1, j} (uint32)
//
// Prints "cases N mismatches M"; exit status 1 when M > 0 or a case leaves the
// reward table's domain (progress 0..2 of a vehicle that is not done).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "driving_vec.h"

using namespace pb;

static uint64_t bits(double x) {
  uint64_t u;
  std::memcpy(&u, &x, sizeof u);
  return u;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  static DrvModel m;
  if (std::fread(&m.g, sizeof(DrvGrid), 1, f) != 1) return 2;
  build_model_tables(m.g, &m);
  std::vector<uint32_t> in;
  uint32_t row[5];
  while (std::fread(row, sizeof row, 1, f) == 1) in.insert(in.end(), row, row + 5);
  std::fclose(f);
  const size_t n = in.size() / 5;
  size_t bad = 0;
  auto fail = [&](const char* what, size_t i) {
    if (bad++ < 20)
      std::printf("case %zu (%08x %08x a %u %u j %u): %s\n", i, in[5 * i], in[5 * i + 1], in[5 * i + 2],
                  in[5 * i + 3], in[5 * i + 4], what);
  };
  for (size_t i = 0; i < n; ++i) {
    const uint32_t s[2] = {in[5 * i], in[5 * i + 1]};
    const uint32_t a0 = in[5 * i + 2], a1 = in[5 * i + 3], j = in[5 * i + 4];
    uint32_t ref[2], got[2];
    drv_step2(m.g, s[0], s[1], (int)a0, (int)a1, j, &ref[0], &ref[1]);
    drv_step2_vec(m, vary(s[0]), vary(s[1]), a0, a1, j, &got[0], &got[1]);
    if (ref[0] != got[0] || ref[1] != got[1]) fail("drv_step2_vec", i);
    for (int v = 0; v < 2; ++v) {
      const uint32_t progress = ((s[v] >> 17) & 127u) - ((ref[v] >> 17) & 127u);
      if (!veh_done(s[v]) && progress > 2u) fail("outside the reward table", i);
      else if (bits(drv_reward(s[v], ref[v])) != bits(drv_reward_vec(m, s[v], ref[v]))) fail("drv_reward_vec", i);
      if (obs_key_serial(m.g, ref[v], ref[1 - v]) != obs_key_vec(m, ref[v], ref[1 - v])) fail("obs_key_vec (next)", i);
      if (obs_key_serial(m.g, s[v], s[1 - v]) != obs_key_vec(m, s[v], s[1 - v])) fail("obs_key_vec (state)", i);
    }
  }
  std::printf("cases %zu mismatches %zu\n", n, bad);
  return bad != 0 || n == 0 ? 1 : 0;
}
