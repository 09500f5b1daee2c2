// The per-pair reset of the I-NTMCP engine (intmcp_reset_pairs) and the episode
// queue of a batch of I-NTMCP episodes (intmcp_episodes_queue_begin, intmcp.h;
// DESIGN.md §17): some pairs of a live batch are left as intmcp_reset leaves
// every pair, while the pairs they share their node slabs with are mid-episode.
// The set of pairs is on the device: an index list and its count.
//
// k_im_clear_pairs  a fixed grid over (listed pair, tree, 16 B word).  Of tree k
//                   of a listed pair it zeroes the node blocks [0, n_nodes[k])
//                   -- node n's 128 B line and its 192 B record group, at
//                   im_node_off / im_rec_delta inside the slab the pair shares
//                   with the other pairs of its wave (a last partial wave's
//                   slabs are B % 64 wide) -- and sets the whole obs-child map
//                   to the empty entry {0, 0, -1}.  No kernel writes a node
//                   block at or beyond n_nodes[k] (ImPair::new_node hands out
//                   every node id, below its counter), so the
//                   blocks beyond stay as the last intmcp_reset left them:
//                   zero.  It reads n_nodes from the headers, so it runs before
//                   the headers are reset.  With fewer (pair, tree) units than
//                   workgroups a unit's words are spread over grid / units
//                   workgroups; with more, a workgroup takes whole units in a
//                   grid stride.
// k_im_reset_pairs  one listed pair per lane: im_reset_pair, the header fields
//                   and node 0 of every tree as k_im_reset writes them (the RNG
//                   counters, seed and tree key carry on).
// k_im_queue_list   one slot per lane, after k_queue_rank: the slots that take a
//                   new entry, in ascending slot order (slot b's place is its
//                   entry minus the first entry handed out this step: no
//                   atomics); their count is k_queue_rank's q.state[1].
// k_im_queue_refill one slot per lane, after the clear: k_queue_refill for
//                   planner pairs.  A finished slot's record goes to rows[its
//                   entry] and fin[b]; with a new entry im_reset_pair, the new
//                   episode's start (episode_reset, the code k_im_episode_reset
//                   runs) and intmcp_episode.h's im_episode_refill: the side
//                   record cleared with parked = 0 and the next update action
//                   -1, which undo the park k_im_episode_step set in this step
//                   (its absorbing bit went with the old root's block).  It
//                   also adds up, per slot, the words the clear stored for it
//                   (intmcp_debug_queue_cleared_bytes: the measurement's figure).
// Plain C++ and 16 B vector stores only; no atomics, no look-back.  Included by
// pomcp_capi.hip after intmcp_episode.hip and pomcp_episode_queue.hip.
#pragma clang fp contract(off)

#include "episode_queue.h"
#include "intmcp_episode.h"

namespace pb {

constexpr int kImClearThreads = 256;
constexpr int kImClearGrid = 2048;                          // 8 workgroups per CU
constexpr int64_t kImLineWords = kImLine / 16;              // 16 B words of a node line
constexpr int64_t kImBlockWords = kImBlock / 16;            // and of a whole block
static_assert(kImLine % 16 == 0 && kImRecs % 16 == 0, "node blocks are cleared in 16 B words");
static_assert(sizeof(IHash) == 16, "an obs-child map slot is one 16 B word");

__global__ __launch_bounds__(kImClearThreads) void k_im_clear_pairs(ImParams p, const int32_t* list,
                                                                    const int32_t* count) {
  int cnt = uni(*count);
  cnt = cnt < 0 ? 0 : cnt > p.B ? p.B : cnt;   // (a count no kernel writes: stay inside the list)
  const int units = cnt * p.nt;                // (pair, tree)
  if (units == 0) return;
  const int G = (int)gridDim.x, wg = (int)blockIdx.x;
  // X workgroups per unit, this one the x-th of unit u0; or whole units, G apart
  const int X = units < G ? G / units : 1;
  const int u0 = wg / X, x = wg - u0 * X;
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  const uint4 empty = make_uint4(0u, 0u, 0u, 0xFFFFFFFFu);   // IHash {okey 0, na 0, child -1}
  for (int u = u0; u < units; u += G) {
    const int b = uni(list[u / p.nt]), k = u % p.nt;
    if (b < 0 || b >= p.B) continue;           // (an index no kernel writes: stay inside the arenas)
    int64_t n = p.hdr[b].n_nodes[k];
    n = n < 0 ? 0 : n > p.Nn ? p.Nn : n;
    char* const line0 = p.nodes + im_node_off(p.Nn, p.B, b, k, 0, p.nt);
    const int64_t ns = im_node_stride(p.B, b), ro = im_rec_delta(p.B, b);
    uint4* const hs = reinterpret_cast<uint4*>(p.hash + ((int64_t)b * p.nt + k) * p.H);
    const int64_t words = n * kImBlockWords, total = words + p.H;
    for (int64_t j = (int64_t)x * kImClearThreads + threadIdx.x; j < total;
         j += (int64_t)X * kImClearThreads) {
      if (j < words) {   // word q of node j / 20: its line's, then its records'
        const int64_t node = j / kImBlockWords, q = j - node * kImBlockWords;
        char* const at = line0 + node * ns + (q < kImLineWords ? q * 16 : ro + (q - kImLineWords) * 16);
        *reinterpret_cast<uint4*>(at) = zero;
      } else {
        hs[j - words] = empty;
      }
    }
  }
}

// k_im_reset's effect on pair b (intmcp.hip; the hash tables and the node
// blocks are k_im_clear_pairs').  The fields are written in place: a private
// copy of the header, indexed by the tree, would live in scratch.
__device__ __forceinline__ void im_reset_pair(const ImParams& p, int b) {
  IHdr& h = p.hdr[b];
  for (int k = 0; k < p.nt; ++k) {
    INode r;
    r.parent = -1;
    r.info = 1u << 4;   // path_ok
    r.visits = 0;
    r.t = 0;
    ICold o;
    o.okey = 0;
    o.stats = -1;
    o.support = kImNoSupport;
    char* const line = p.nodes + im_node_off(p.Nn, p.B, b, k, 0, p.nt);
    *reinterpret_cast<INode*>(line) = r;
    *reinterpret_cast<ICold*>(line + kImCold) = o;
    h.n_nodes[k] = 1;
    h.n_stats[k] = 0;
    h.n_log[k] = 0;
    h.mm_max[k] = p.has_kb ? p.kb_max : -__builtin_inf();
    h.mm_min[k] = p.has_kb ? p.kb_min : __builtin_inf();
  }
  h.cur = 0;
  h.root_sel = 0;
  h.root_size = 0;
  h.sup_sel = 0;
  h.n_sup = 0;
  h.sup_used = 0;
  h.err = 0;
  h.last_action = -1;
  h.num_sims = 0;
  h.search_depth = 0;
  h.sims_done = 0;
  h.pad = 0;
  for (int m = 0; m < kImMaxMid; ++m) {
    h.msel[m] = 0;
    h.n_msup[m] = 0;
    h.msup_used[m] = 0;
    h.mpad[m] = 0;
  }
}

__global__ __launch_bounds__(64) void k_im_reset_pairs(ImParams p, const int32_t* list,
                                                       const int32_t* count) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int cnt = *count;
  if (i >= cnt || i >= p.B) return;
  const int b = list[i];
  if (b < 0 || b >= p.B) return;
  im_reset_pair(p, b);
}

__global__ __launch_bounds__(kEpThreads) void k_im_queue_list(EpQueueDev q, int32_t* list, int B) {
  const int b = (int)(blockIdx.x * kEpThreads + threadIdx.x);
  if (b >= B) return;
  const int32_t a = q.assign[b];
  if (a < 0) return;
  const int32_t at = a - (q.state[0] - q.state[1]);   // (state: the new next, the entries handed out)
  if (at >= 0 && at < B) list[at] = b;
}

template <class E>
__global__ __launch_bounds__(kEpThreads) void k_im_queue_refill(ImParams p, EpDev ep, EpQueueDev q,
                                                                intmcp_episode_kept* kept,
                                                                int64_t* cleared) {
  __shared__ typename E::Model sm;
  stage_model(p.model, sm);
  const int b = (int)(blockIdx.x * kEpThreads + threadIdx.x);
  if (b >= p.B) return;
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
    row->policy_index = ep.ps[b].policy_index;   // (-1 without a population)
    row->start_step = q.slot_start[b];
    // (row->acc stays as intmcp_episodes_queue_begin zeroed it: no belief accuracy)
    q.slot_q[b] = a;   // (kQueueRetire: the pair stays parked as k_im_episode_step left it)
    intmcp_episode_kept k = kept[b];
    int32_t next;
    if (im_episode_refill(a, &k, &next)) {
      // (measurement: the 16 B words k_im_clear_pairs stored for this slot so far)
      int64_t words = 0;
      for (int t = 0; t < p.nt; ++t) {
        const int64_t n = p.hdr[b].n_nodes[t];
        words += (n < 0 ? 0 : n > p.Nn ? p.Nn : n) * kImBlockWords + p.H;
      }
      cleared[b] += words;
      im_reset_pair(p, b);
      pomcp_episode_state ns;
      pomcp_episode_pop_state r;
      const uint64_t key = episode_reset<E>(sm, im_episode_ego(p), q.seeds[a], ep.pop, &ns, &r);
      ep.st[b] = ns;
      ep.ps[b] = r;
      ep.in_obs[b] = key;
      kept[b] = k;
      q.slot_ord[b] += 1;
      q.slot_start[b] = q.step + 1;
    }
    if (next != kImEpKeepInput) ep.in_actions[b] = next;
  }
  q.fin_q[b] = fq;
}

// Test-only (intmcp_debug_arena_scan): of one tree of one pair, the node blocks
// in [0, Nn) that hold a non-zero byte, one past the highest such block, and
// the occupied obs-child map slots (any slot that is not the empty entry).
// One workgroup: slow on purpose-built arenas, fine for the tests'.
__global__ __launch_bounds__(256) void k_im_arena_scan(ImParams p, int b, int k,
                                                       unsigned long long* out) {
  __shared__ unsigned long long part[3][256];
  const int t = (int)threadIdx.x;
  const char* const line0 = p.nodes + im_node_off(p.Nn, p.B, b, k, 0, p.nt);
  const int64_t ns = im_node_stride(p.B, b), ro = im_rec_delta(p.B, b);
  unsigned long long used = 0ull, top = 0ull, slots = 0ull;
  for (int64_t n = t; n < p.Nn; n += 256) {
    const uint4* const l = reinterpret_cast<const uint4*>(line0 + n * ns);
    const uint4* const r = reinterpret_cast<const uint4*>(line0 + n * ns + ro);
    uint32_t any = 0u;
    for (int i = 0; i < (int)kImLineWords; ++i) any |= l[i].x | l[i].y | l[i].z | l[i].w;
    for (int i = 0; i < (int)(kImBlockWords - kImLineWords); ++i) any |= r[i].x | r[i].y | r[i].z | r[i].w;
    if (any != 0u) {
      used += 1ull;
      top = (unsigned long long)(n + 1);
    }
  }
  const IHash* const hs = p.hash + ((int64_t)b * p.nt + k) * p.H;
  for (int64_t s = t; s < p.H; s += 256) {
    const IHash e = hs[s];
    if (e.child != -1 || e.na != 0u || e.okey != 0ull) slots += 1ull;
  }
  part[0][t] = used;
  part[1][t] = top;
  part[2][t] = slots;
  __syncthreads();
  if (t == 0) {
    unsigned long long a = 0ull, m = 0ull, c = 0ull;
    for (int i = 0; i < 256; ++i) {
      a += part[0][i];
      m = part[1][i] > m ? part[1][i] : m;
      c += part[2][i];
    }
    out[0] = a;
    out[1] = m;
    out[2] = c;
  }
}

}  // namespace pb
