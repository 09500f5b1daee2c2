// The episode queue of a batch of episodes (pomcp_episodes_queue_begin,
// pomcp.h): a finished tree takes the next environment seed of a
// device-resident queue instead of staying parked, with nothing per tree on
// the host between steps.  Launched by pomcp_episodes_step while a queue is
// active, after k_episode_step (and k_episode_belief_acc) and before
// k_episode_live:
//
// k_queue_rank    one workgroup.  Ranks the slots whose episode finished this
//                 step in ascending slot order (tiles of kRankThreads slots in
//                 order; within a tile ballots and a fixed-order sum of the
//                 waves' counts: integers, the same on every run) and writes
//                 every slot's decision (episode_queue.h queue_assign: an entry,
//                 retire, or play on), the new `next` and the number of slots
//                 refilled.
// k_queue_refill  one slot per lane.  A finished slot's record goes out to
//                 rows[its entry] and to fin[b] (the record of the episode that
//                 just ended, for on_step observers).  With a new entry the tree
//                 is reset as k_reset resets it -- the header fields, the
//                 overflow map's generation (the map cleared when the counter
//                 wraps), the RNG stream counters carried on -- except that the
//                 wave's shared log count (wlog) is left alone; the new episode
//                 starts (episode_reset, the code k_episode_reset runs) and the
//                 tree's bit is set in its search wave's drop mask.  A
//                 256-lane workgroup holds four search waves' trees, one per
//                 hardware wave, so a mask is one __ballot, stored by lane 0:
//                 every wave's mask is rewritten on every step, no atomics.
// k_log_drop      one workgroup per search wave's log.  Returns at once for a
//                 zero mask; otherwise a stable in-place compaction that drops
//                 the records whose lane tag is in the mask (the refilled
//                 trees' records of their previous episode) while the wave's
//                 other trees are mid-episode.  A pass loads kDropRecs records
//                 per thread, then a workgroup barrier, then ranks the kept
//                 ones (ballots + a fixed-order sum of the waves' counts) and
//                 stores them; a kept record lands at or before its own place
//                 and every place a pass writes lies before every record a
//                 later pass reads, so filtering in place is safe
//                 (k_compact_log's argument).  wlog[wave] ends as the kept count.
// Plain C++ and vector stores only; no global atomics, no look-back.
// Included by pomcp_capi.hip.
#pragma clang fp contract(off)

#include "envs.h"
#include "episode_queue.h"
#include "episode_step.h"
#include "pomcp_device.h"

namespace pb {

static_assert(kLogLaneShift == kIdBits, "a log record's lane tag");
static_assert(sizeof(pomcp_episode_queue_row) == 128, "queue row layout");
static_assert(kEpThreads % kWave == 0, "a refill wave is one search wave's trees");

constexpr int kRankThreads = 1024;
// k_log_drop: 16 waves as k_compact_log (one workgroup per CU streams a log),
// 2 records per thread and pass
constexpr int kDropThreads = 1024;
constexpr int kDropRecs = 2;
constexpr int kDropPass = kDropThreads * kDropRecs;

struct EpQueueDev {
  const uint64_t* seeds;            // [n] the queue
  pomcp_episode_queue_row* rows;    // [n] results, in queue order
  int32_t* slot_q;                  // [B] the entry each slot plays (kQueueRetire: retired)
  int32_t* slot_ord;                // [B] its ordinal among the slot's episodes
  int32_t* slot_start;              // [B] the batch step it started at
  int32_t* assign;                  // [B] this step's decisions (k_queue_rank)
  int32_t* state;                   // [2] {next, slots refilled this step}
  uint64_t* drop;                   // [search waves] lanes whose records k_log_drop drops
  pomcp_episode_state* fin;         // [B] the records of the episodes that ended this step
  int32_t* fin_q;                   // [B] their entries (-1: none ended in the slot)
  const pomcp_episode_belief_acc* acc_in;   // [B] (k_episode_belief_acc's), or null
  pomcp_episode_belief_acc* acc;    // the same, to be cleared
  int32_t n;                        // queue length
  int32_t step;                     // the batch step being finished (0, 1, ...)
};

__global__ __launch_bounds__(kRankThreads) void k_queue_rank(EpDev ep, EpQueueDev q, int B) {
  constexpr int kW = kRankThreads / kWave;
  __shared__ int32_t wsum[kW];
  const int t = (int)threadIdx.x, w = t >> 6, lane = lane_id();
  const int32_t next = q.state[0];
  int32_t done = 0;   // finished slots before this tile
  for (int base = 0; base < B; base += kRankThreads) {
    const int b = base + t;
    const bool f = b < B && queue_slot_finished(q.slot_q[b], ep.st[b].finished);
    const uint64_t m = __ballot(f);
    if (lane == 0) wsum[w] = __popcll(m);
    __syncthreads();
    int pre = 0, tot = 0;
#pragma unroll
    for (int v = 0; v < kW; ++v) {
      pre += v < w ? wsum[v] : 0;
      tot += wsum[v];
    }
    __syncthreads();   // (wsum is rewritten by the next tile)
    if (b < B) {
      const int32_t rank = done + pre + __popcll(m & ((1ull << lane) - 1ull));
      q.assign[b] = f ? queue_assign(rank, next, q.n) : kQueuePlaying;
    }
    done += tot;
  }
  if (t == 0) {
    const int32_t r = queue_refilled(done, next, q.n);
    q.state[0] = next + r;
    q.state[1] = r;
  }
}

// k_reset's effect on one tree, by one lane, but for the wave's shared log
// count; true: the overflow map's generation wrapped and the map is to be
// cleared (clear_ovf, by the whole wave).
__device__ __forceinline__ bool queue_reset_tree(const DevParams& p, int tree) {
  TreeHdr h = p.hdr[tree];
  int epoch = (h.epoch + 1) & (int)kEpochMask;
  const bool wrapped = epoch == 0;
  if (wrapped) epoch = 1;
  h.n_blocks = 0;
  h.n_log = 0;
  h.n_nodes = 1;
  h.error = 0;
  h.belief_size = 0;
  h.epoch = epoch;
  h.root_t = 0;
  h.root_id = kRootId;
  h.root_blk = -1;
  h.root_visits = 0;
  h.root_abs = 0;
  h.mm_max = p.has_kb ? p.kb_max : -__builtin_inf();   // utils.py:21-27
  h.mm_min = p.has_kb ? p.kb_min : __builtin_inf();
  p.hdr[tree] = h;
  return wrapped;
}

template <class E>
__global__ __launch_bounds__(kEpThreads) void k_queue_refill(DevParams p, EpDev ep, EpQueueDev q) {
  __shared__ typename E::Model sm;
  stage_model(p.model, sm);
  const int b = (int)(blockIdx.x * kEpThreads + threadIdx.x);
  const int lane = lane_id();
  const int wave0 = uni(b - lane);   // the first tree of this lane's search wave
  if (wave0 >= p.B) return;          // (whole waves leave: the ballots below are complete)
  bool refill = false, wrapped = false;
  if (b < p.B) {
    const int32_t a = q.assign[b];
    int32_t fq = -1;
    if (a != kQueuePlaying) {
      const int32_t at = q.slot_q[b];
      const pomcp_episode_state s = ep.st[b];
      fq = at;
      q.fin[b] = s;
      pomcp_episode_queue_row* const row = q.rows + at;
      row->res = s.res;
      row->slot = b;
      row->slot_order = q.slot_ord[b];
      row->policy_index = ep.ps != nullptr ? ep.ps[b].policy_index : -1;
      row->start_step = q.slot_start[b];
      // (without tracking the rows' records stay as pomcp_episodes_queue_begin zeroed them)
      if (q.acc_in != nullptr) row->acc = q.acc_in[b];
      q.slot_q[b] = a;   // (kQueueRetire: the tree stays parked as k_episode_step left it)
      if (a >= 0) {
        refill = true;
        wrapped = queue_reset_tree(p, b);
        pomcp_episode_state ns;
        pomcp_episode_pop_state r;
        const uint64_t key = episode_reset<E>(sm, p.ego, q.seeds[a], ep.pop, &ns, &r);
        ep.st[b] = ns;
        if (ep.ps != nullptr) ep.ps[b] = r;
        ep.in_obs[b] = key;
        ep.in_actions[b] = -1;
        if (ep.states != nullptr) ep.states[b] = make_uint2(ns.v0, ns.v1);
        uint4* const ko = reinterpret_cast<uint4*>(ep.kept + b);
        for (int k = 0; k < (int)(sizeof(pomcp_root_stats) / 16); ++k) ko[k] = make_uint4(0, 0, 0, 0);
        if (q.acc != nullptr) {
          uint4* const ao = reinterpret_cast<uint4*>(q.acc + b);
          ao[0] = make_uint4(0, 0, 0, 0);
          ao[1] = make_uint4(0, 0, 0, 0);
        }
        q.slot_ord[b] += 1;
        q.slot_start[b] = q.step + 1;
      }
    }
    q.fin_q[b] = fq;
  }
  const uint64_t mask = __ballot(refill);
  if (lane == 0) q.drop[wave0 / kWave] = mask;
  // (rare: once in kEpochMask resets of a tree) the wrapped trees' maps, one
  // after the other by the whole wave
  uint64_t wr = __ballot(wrapped);
  while (wr != 0ull) {
    const int l = __builtin_ctzll(wr);
    clear_ovf(p, wave0 + l, lane);
    wr &= wr - 1ull;
  }
}

__global__ __launch_bounds__(kDropThreads) void k_log_drop(DevParams p, const uint64_t* masks) {
  constexpr int kW = kDropThreads / kWave;
  constexpr int R = kDropRecs;
  __shared__ int32_t wsum[R][kW];
  const int sw = (int)blockIdx.x;
  const uint64_t mask = uni64(masks[sw]);
  if (mask == 0ull) return;
  const int t = (int)threadIdx.x, w = t >> 6, lane = lane_id();
  const WaveLog wl(p.plog, p.Np, sw, p.tm);
  const uint32_t cap = (uint32_t)(kWave * p.Np);   // (< 2^32: pomcp_create)
  const uint32_t cnt = uniu(p.wlog[sw]);
  const uint32_t n = cnt < cap ? cnt : cap;   // (a count no kernel writes: stay inside the log)
  const bool tm = p.tm != 0;
  const uint64_t below = (1ull << lane) - 1ull;
  uint32_t out = 0u;
  for (uint32_t base = 0u; base < n; base += (uint32_t)kDropPass) {
    LogRec r[R];
    uint32_t aux[R];
    bool keep[R];
    uint64_t mk[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {   // sub-pass j: record base + j T + thread
      const uint32_t i = base + (uint32_t)(j * kDropThreads + t);
      r[j] = LogRec{0u, 0u, 0u};
      aux[j] = 0u;
      if (i < n) {
        r[j] = wl.load(i);
        if (tm) aux[j] = wl.aux[i];
      }
      keep[j] = i < n && log_drop_keeps(r[j].id, mask);
      mk[j] = __ballot(keep[j]);
      if (lane == 0) wsum[j][w] = __popcll(mk[j]);
    }
    __syncthreads();   // every record of the pass is loaded before one is stored
    uint32_t tot = 0u;
#pragma unroll
    for (int j = 0; j < R; ++j) {
      int pre = 0, tj = 0;
#pragma unroll
      for (int v = 0; v < kW; ++v) {
        pre += v < w ? wsum[j][v] : 0;
        tj += wsum[j][v];
      }
      const uint32_t i = base + (uint32_t)(j * kDropThreads + t);
      const uint32_t at = out + tot + (uint32_t)(pre + __popcll(mk[j] & below));
      if (keep[j] && at != i) {   // (the records before the first dropped one stay)
        wl.store(at, r[j]);
        if (tm) wl.aux[at] = aux[j];
      }
      tot += (uint32_t)tj;
    }
    out += tot;
    __syncthreads();   // (wsum is rewritten by the next pass)
  }
  if (t == 0) p.wlog[sw] = out;
}

}  // namespace pb
