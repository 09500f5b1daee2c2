// k_belief_stats: per-tree counts over the current root belief -- the device
// side of BeliefStatTracker (utils.py:292-339; pomcp_belief_stats, pomcp.h).
//
// A tree's belief is hdr[b].belief_size records {t, v0, v1, aux} of its Nr-record
// region (pomcp_device.h bel_at): [0, n) when belief_sel == 0, [Nr - n, Nr) when
// it is 1.  Counts do not depend on particle order, so the range is read in
// ascending address order whichever end it sits at.
//
// One 256-thread workgroup per tree, trees grid-strided.  Each lane loads one
// 16 B record per pass (1 KB coalesced per wave instruction); a wave counts with
// __ballot + __popcll into wave-uniform accumulators; the four waves' partial
// counts meet in LDS and thread 0 stores the tree's record.  Integers only, no
// global atomics, no pre-zeroed output: the result is the same on every run.
// Included by pomcp_capi.hip.
#include "belief_stats.h"
#include "pomcp_device.h"

namespace pb {

constexpr int kBelThreads = 256;
constexpr int kBelWaves = kBelThreads / kWave;
constexpr int kBelMaxGrid = 2048;
constexpr int kBelWords = 2 + kTmMax;   // matches, bad-aux flag, policy histogram
static_assert(kTmMax == POMCP_MAX_TYPE_POLICIES, "histogram width");
static_assert(sizeof(pomcp_belief_counts) == 4 * (4 + POMCP_MAX_TYPE_POLICIES), "counts layout");

// The counts of the n records at `rec`, made by the whole workgroup: every
// thread calls it with the same arguments; after its barrier red[w][] holds
// wave w's counts ({matches, bad-aux flag, histogram}), which one thread adds up
// with bel_totals.  The last group of a wave may be partial: its lanes past n
// load nothing and classify as 0 (masked, not padded).  `red` is reused by the
// next call: the caller puts a __syncthreads() between two calls.
__device__ __forceinline__ void bel_count_block(const uint4* rec, int n, uint32_t q0, uint32_t q1,
                                                int has_q, int num_other, int lane, int wave,
                                                int32_t (*red)[kBelWords]) {
  int32_t matches = 0, bad = 0;
  int32_t hist[kTmMax];
#pragma unroll
  for (int j = 0; j < kTmMax; ++j) hist[j] = 0;
  for (int64_t i0 = (int64_t)wave * kWave; i0 < n; i0 += kBelThreads) {
    const int64_t i = i0 + lane;
    const bool live = i < n;
    uint32_t c = 0u;
    if (live) {
      const uint4 r = rec[i];
      c = bel_classify(r.y, r.z, r.w, q0, q1, has_q, (uint32_t)num_other);
    }
    matches += (int32_t)__popcll(__ballot((c & kBelMatch) != 0u));
    if (num_other > 0) {
      bad |= __ballot((c & kBelBadAux) != 0u) != 0ull ? 1 : 0;
      // a bad aux never reaches the histogram: its class is not counted
      const bool ok = live && (c & kBelBadAux) == 0u;
      const int pol = (int)(c >> kBelPolShift);
#pragma unroll
      for (int j = 0; j < kTmMax; ++j)
        if (j < num_other) hist[j] += (int32_t)__popcll(__ballot(ok && pol == j));
    }
  }
  if (lane == 0) {
    red[wave][0] = matches;
    red[wave][1] = bad;
#pragma unroll
    for (int j = 0; j < kTmMax; ++j) red[wave][2 + j] = hist[j];
  }
  __syncthreads();
}

__device__ __forceinline__ void bel_totals(const int32_t (*red)[kBelWords],
                                           int32_t tot[kBelWords]) {
#pragma unroll
  for (int k = 0; k < kBelWords; ++k) {
    int32_t t = 0;
#pragma unroll
    for (int w = 0; w < kBelWaves; ++w) t += red[w][k];
    tot[k] = t;
  }
}

// q: [B] query states (v0, v1), or null.  num_other: 0 on plain contexts (aux
// is not looked at), else the number of other-agent policies.
__global__ __launch_bounds__(kBelThreads) void k_belief_stats(DevParams dp, const uint2* q,
                                                              int num_other,
                                                              pomcp_belief_counts* out) {
  __shared__ int32_t red[kBelWaves][kBelWords];
  const int lane = lane_id();
  const int wave = uni((int)threadIdx.x / kWave);
  for (int b = (int)blockIdx.x; b < dp.B; b += (int)gridDim.x) {
    const TreeHdr* h = dp.hdr + b;
    int n = uni(h->belief_size);
    const int sel = uni(h->belief_sel);
    int err = uni(h->error);
    if (n < 0 || (int64_t)n > dp.Nr) {   // a header no kernel writes: read nothing
      n = 0;
      if (err == 0) err = POMCP_E_INVALID;
    }
    const uint4* rec = dp.belief + (int64_t)b * dp.Nr + (sel ? dp.Nr - n : 0);
    const int has_q = q != nullptr;
    uint32_t q0 = 0u, q1 = 0u;
    if (has_q) {
      const uint2 s = q[b];
      q0 = uniu(s.x);
      q1 = uniu(s.y);
    }
    bel_count_block(rec, n, q0, q1, has_q, num_other, lane, wave, red);
    if (threadIdx.x == 0) {
      int32_t tot[kBelWords];
      bel_totals(red, tot);
      if (tot[1] != 0 && err == 0) err = POMCP_E_INVALID;
      int4* o = reinterpret_cast<int4*>(out + b);
      o[0] = make_int4(n, has_q ? tot[0] : -1, err, 0);
      o[1] = make_int4(tot[2], tot[3], tot[4], tot[5]);
      o[2] = make_int4(tot[6], tot[7], tot[8], tot[9]);
    }
    __syncthreads();   // red is reused by the next tree
  }
}

}  // namespace pb
