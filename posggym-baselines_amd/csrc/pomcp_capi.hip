// C-ABI host side of libpomcp_hip.so (include/pomcp.h).
//
// Owns every device allocation of a planner batch, validates the
// MCTSConfig-derived parameters (config.py:33-55 asserts) and launches the
// kernels of pomcp_kernels.hip on one HIP stream.
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

// Single translation unit: the kernels are compiled together with their launchers.
#include "pomcp_kernels.hip"
// the host-only entry points (environment models, RNG words, log / exp tables):
// plain C++, also built on its own with the host sanitizers (tests/test_host_sanitize.py)
#include "host_api.cpp"
#include "belief_stats.hip"
#include "pomcp_episode.hip"
#include "pomcp_episode_group.hip"   // (after pomcp_episode.hip's EpDev)
#include "episode_belief_acc.hip"
#include "pomcp_episode_queue.hip"
#include "pomcp_episode_group_queue.hip"   // (after both: EpGroupDev, EpQueueDev)
#include "pomcp_search.hip"
#include "pomcp_search_lds.hip"
#include "../../include/intmcp.h"   // (INTMCP_MAX_TREES)
#include "intmcp.hip"
#include "intmcp_episode.hip"   // (after ImParams and pomcp_episode.hip's EpDev)
#include "intmcp_episode_queue.hip"   // (after pomcp_episode_queue.hip's EpQueueDev)
#include "../../include/pomcp_debug.h"
#include "host_ctx.h"
#include "host_episodes.h"

using namespace pb;

// k_search lives in pomcp_search_tu.hip (a translation unit of its own)
// (dl: its compile-time depth limit, the units of pomcp_search_dl_tu.hip; 0: the generic kernel)
const void* pb_search_kernel(int row, int e, int sel, int dl);

static_assert(sizeof(pomcp_grid) == sizeof(DrvGrid), "grid layout");
static_assert(sizeof(pomcp_pe_grid) == 1344, "pe grid layout");
static_assert(sizeof(Line) == 128, "block line layout");
static_assert(sizeof(OvfSlot) == 32, "overflow slot layout");

struct pomcp_ctx : HostCtx, EpisodeHost {
  pomcp_config cfg;
  DevParams dp{};
  bool have_snapshot = false;
  TreeHdr* snap_hdr = nullptr;
  std::vector<int32_t> host_upd;
  std::vector<pomcp_root_stats> host_stats;
  pomcp_merged_root* merged = nullptr;   // [B] device results of pomcp_merge_roots
  double* gather = nullptr;              // [gather_world][B][R] pomcp_root_gather_buffer
  int gather_world = 0;
  int search_kind = POMCP_SEARCH_AUTO;
  TmTables host_tm{};                    // type-based contexts (pomcp_set_type_policies)
  TmEgo host_tme{};                      // their ego policies' kinds (pomcp_set_type_ego_kinds)
  bool tm_set = false;
  // a lane search with deferred cut-off records ran since the last update /
  // reset / restore: the mode and the kernel stay fixed until the re-root
  // materialises those children (a record's absorbing flag must not race an
  // eager arrival's, mcts.py:370)
  bool defer_pending = false;
  // the re-root's log scan: the streaming kernels (k_log_filter + the
  // materialising pass) unless POMCP_LOG_SCAN=legacy (one workgroup per log,
  // k_compact_log: A/B and fallback); the look-back tags' epoch
  bool log_scan_legacy = false;
  bool lf_packed_cmap = true;   // POMCP_LF_PACKED_CMAP=off: tests only
  uint32_t lf_epoch = 0;
  int lf_grid = 0;
  // some tree has had a root since the last reset (pomcp_update /
  // pomcp_set_root_belief): pomcp_belief_stats has a belief to count
  bool have_root = false;
  pomcp_belief_counts* bel_out = nullptr;   // [B] device results of k_belief_stats
  uint2* bel_q = nullptr;                   // [B] its query states
  // batched episodes (pomcp_episodes_begin / _step; EpisodeHost holds the batch,
  // the population and the queue): whether the true states are tracked in bel_q
  bool ep_track = false;
  // belief accuracy on the device (pomcp_episodes_track_belief_acc): what the
  // next begin turns on, whether the running batch tracks, its device state
  bool ep_acc_want = false, ep_acc_steps_want = false;
  bool ep_acc = false;
  EpAccDev acc{};
  double* acc_steps_buf = nullptr;            // the per-step table and its capacity (doubles)
  int64_t acc_steps_cap = 0;
  double host_other_pi[kTmMax][POMCP_MAX_ACTIONS] = {};   // pomcp_type_policies.other_pi
  double ep_acc_ms = 0.0;   // k_episode_belief_acc's device time, between its two events
  hipEvent_t acc_ev[2] = {nullptr, nullptr};
  // the episode queue's (q.drop; q_ms = {rank + refill, k_log_drop}, q_ev[0 .. 2])
  uint64_t* drop_masks = nullptr;   // [search waves] (also pomcp_debug_log_drop's)
  // root-parallel planners (pomcp_episodes_set_group): the group size the next
  // begin takes, the running batch's (1: one episode per tree) and its device
  // state; the kept merged records, [num_trees / 2] (the most groups there are)
  int32_t ep_group_want = 1;
  int32_t ep_group = 1;
  EpGroupDev gr{};
  pomcp_merged_root* ep_kept_merged = nullptr;
  // the episode queue of groups (pomcp_episodes_group_queue_begin): the running
  // queue's slots are the batch's groups; its device state, [num_trees / 2] each
  bool gq_active = false;
  EpGroupQueueDev gq{};
};

// Wave-per-tree search (k_search_lds) for batches up to this many trees: one
// tree per CU at a time, so beyond one round of 256 trees the tree-per-lane
// kernel's throughput wins (DESIGN.md §6, 65,536 simulations per tree: 256
// trees 44.7 M vs ~24 M simulations/s; 1,024 trees would run four rounds,
// ~45 M, vs 86-95 M).
constexpr int kWaveSearchMaxTrees = 256;
// and only while its per-tree scratch log stays small
constexpr int64_t kWaveSearchMaxScratch = (int64_t)4 << 30;
// step-tree producers for depth limits up to this (use_step_tree)
constexpr int kStepTreeMaxDepth = 8;

// f(Env{}) with the context's environment (envs.h)
template <class F>
static void with_env(const pomcp_ctx* ctx, F&& f) {
  env_dispatch4<EnvDriving, EnvPursuitEvasion, EnvCoopReaching, EnvPredatorPrey>(ctx->dp.env, f);
}

// f(Env{}) with the context's environment as the episode kernels know it (episode_step.h)
template <class F>
static void with_episode_env(const pomcp_ctx* ctx, F&& f) {
  env_dispatch4<EpDriving, EpPursuitEvasion, EpCoopReaching, EpPredatorPrey>(ctx->dp.env, f);
}

// The first tree whose status code(t) is an error, named by its kind.
template <class Code>
static int first_tree_error(pomcp_ctx* ctx, const char* what, Code code) {
  return first_error(ctx, ctx->dp.B, code, [&](int t, int e) {
    const char* kind = e == POMCP_E_ARENA ? "arena capacity exceeded"
                       : e == POMCP_E_NOT_FOUND ? "root has no child node for action"
                       : e == POMCP_E_STATE ? "call out of order"
                       : e == POMCP_E_INVALID ? "invalid observation"
                                              : "error";
    return std::string(what) + ": tree " + std::to_string(t) + ": " + kind;
  });
}

static unsigned grid_blocks(int B) { return (unsigned)((B + kTreesPerBlock - 1) / kTreesPerBlock); }
static unsigned search_blocks(int B) { return (unsigned)((B + kTPB - 1) / kTPB); }
// Workgroup size of a search launch: one-wave workgroups while the launch has
// at most 3 waves per CU (3 such workgroups fit a CU's LDS: root cache 35 KB +
// model tables each), so a small launch's waves spread over all 256 CUs; a
// full launch uses 256-lane workgroups, one per CU.
static int search_tpb(int B) { return (B + kWave - 1) / kWave <= 3 * 256 ? kTPBSmall : kTPB; }
static int search_waves(int B) { return (B + kWave - 1) / kWave; }

extern "C" {

int32_t pomcp_abi_version(void) { return POMCP_ABI_VERSION; }

const char* pomcp_last_error(const pomcp_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int pomcp_set_stream(pomcp_ctx* ctx, void* hip_stream) {
  if (!ctx) return POMCP_E_INVALID;
  if (hip_stream) {
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
    ctx->stream = (hipStream_t)hip_stream;
    ctx->own_stream = false;
  }
  return POMCP_OK;
}

// (desc: the description beside the config, pomcp_create_env (the env_id's
// struct, its size checked there); null from pomcp_create)
static int validate(const pomcp_config* c, const void* desc, std::string* why) {
  const pomcp_cr_grid* cr = static_cast<const pomcp_cr_grid*>(desc);
  auto bad = [&](const char* m) {
    *why = m;
    return POMCP_E_INVALID;
  };
  if (c->abi_version != POMCP_ABI_VERSION) return bad("ABI version mismatch");
  if (c->env_id == POMCP_ENV_COOPERATIVE_REACHING && cr == nullptr) {
    *why = "env_id: CooperativeReaching-v0 takes its pomcp_cr_grid through pomcp_create_env";
    return POMCP_E_UNSUPPORTED;
  }
  if (c->env_id == POMCP_ENV_PREDATOR_PREY && desc == nullptr) {
    *why = "env_id: PredatorPrey-v0 takes its pomcp_pp_grid through pomcp_create_env";
    return POMCP_E_UNSUPPORTED;
  }
  if (c->env_id != POMCP_ENV_DRIVING && c->env_id != POMCP_ENV_PURSUIT_EVASION &&
      c->env_id != POMCP_ENV_COOPERATIVE_REACHING && c->env_id != POMCP_ENV_PREDATOR_PREY) {
    *why = "env_id: Driving-v1, PursuitEvasion-v1, CooperativeReaching-v0 or PredatorPrey-v0";
    return POMCP_E_UNSUPPORTED;
  }
  if (c->num_agents != 2) { *why = "the engine's models are 2-agent"; return POMCP_E_UNSUPPORTED; }
  if (c->num_actions != (c->env_id == POMCP_ENV_PURSUIT_EVASION ? 4 : 5)) return bad("num_actions of the model");
  if (c->env_id == POMCP_ENV_COOPERATIVE_REACHING && !cr_grid_ok(*cr))
    return bad("cr grid: size 3..8, four corner goals, obs_distance -1..7");
  if (c->env_id == POMCP_ENV_PREDATOR_PREY && !pp_grid_ok(*static_cast<const pomcp_pp_grid*>(desc)))
    return bad("pp grid: size 5 or 10, 1..3 prey, prey_strength 1..2, obs_dim 1..2, the start "
               "cells and the capture reward of the model");
  if (c->env_id == POMCP_ENV_PURSUIT_EVASION) {
    const pomcp_pe_grid& g = c->pe_grid;
    if (g.width < 1 || g.width > 16 || g.height < 1 || g.height > 16) return bad("pe grid size");
    if (g.n_evader_start < 1 || g.n_evader_start > 4 || g.n_pursuer_start < 1 ||
        g.n_pursuer_start > 4 || g.n_goal < 1 || g.n_goal > 4)
      return bad("pe starts / goals (1..4 each)");
    if (g.max_obs_distance < 0 || g.max_obs_distance > 15) return bad("max_obs_distance 0..15");
    if (!(g.reward_norm > 0.0)) return bad("reward_norm > 0");
  }
  if (c->ego_agent < 0 || c->ego_agent >= c->num_agents) return bad("ego_agent out of range");
  if (c->num_actions < 1 || c->num_actions > POMCP_MAX_ACTIONS) return bad("num_actions");
  if (c->action_selection < 0 || c->action_selection > 2) return bad("action_selection");
  if (!(c->discount >= 0.0 && c->discount <= 1.0)) return bad("discount in [0,1]");
  if (!(c->c > 0.0)) return bad("c > 0");
  if (!(c->pucb_exploration_fraction >= 0.0 && c->pucb_exploration_fraction <= 1.0))
    return bad("pucb_exploration_fraction in [0,1]");
  if (!(c->reinvigoration_sample_limit_factor >= 1.0)) return bad("sample_limit_factor >= 1");
  if (c->depth_limit < 0 || c->step_limit < 0) return bad("depth/step limit");
  if (c->num_particles < 1 || c->extra_particles < 0) return bad("num_particles");
  if (c->num_trees < 1) return bad("num_trees >= 1");
  if (c->type_based != 0 && c->type_based != 1) return bad("type_based is 0 or 1");
  if (c->max_blocks < 1 || c->max_blocks * blk_lines(c->num_actions, c->type_based) * 128 > INT32_MAX)
    return bad("max_blocks");
  if (c->num_actions < 2 || c->num_actions > kMaxA) { *why = "the search kernel supports 2 to 5 actions"; return POMCP_E_UNSUPPORTED; }
  if (c->max_particles < 1 || c->max_particles * kWave > UINT32_MAX) return bad("max_particles");
  // ids: inline slots (max_blocks * A * 6), overflow entries, deferred records
  // (max_blocks * A, pomcp_device.h)
  if (c->max_blocks * c->num_actions * (kSlots + 1) + 1 + c->overflow_slots >= (int64_t)kIdMask)
    return bad("obs node ids exceed 2^26 (max_blocks * A * 7 + overflow_slots)");
  // max_belief: the root belief region (the root belief and the next, one from
  // each end: pomcp_device.h bel_at)
  if (c->max_belief < 2 * (c->num_particles + c->extra_particles)) return bad("max_belief too small");
  if (c->max_belief > INT32_MAX) return bad("max_belief < 2^31");
  if (c->overflow_slots < kBucket || (c->overflow_slots & (c->overflow_slots - 1)) != 0 ||
      c->overflow_slots > (1ll << 28))
    return bad("overflow_slots must be a power of two in [16, 2^28]");
  if (!c->log_table || c->log_table_size < 2) return bad("log_table");
  if (!c->discount_pow || c->discount_pow_size < 1) return bad("discount_pow");
  if (c->env_id != POMCP_ENV_DRIVING) return POMCP_OK;
  const pomcp_grid& g = c->grid;
  if (g.width < 1 || g.width > 16 || g.height < 1 || g.height > 16) return bad("grid size");
  if (g.num_locs < 2 || g.num_locs > 8) return bad("grid locations");
  const int ncells = (g.obs_front + g.obs_back + 1) * (2 * g.obs_side + 1);
  if (g.obs_front < 0 || g.obs_back < 0 || g.obs_side < 0 || ncells > 15)
    return bad("obs window must have <= 15 cells");
  return POMCP_OK;
}

static int create_ctx(const pomcp_config* cfg, const void* desc, int32_t device, void* hip_stream,
                      pomcp_ctx** out);

int pomcp_create(const pomcp_config* cfg, int32_t device, void* hip_stream, pomcp_ctx** out) {
  return create_ctx(cfg, nullptr, device, hip_stream, out);
}

int pomcp_create_env(const pomcp_config* cfg, const void* env_desc, int64_t env_desc_bytes,
                     int32_t device, void* hip_stream, pomcp_ctx** out) {
  if (!cfg || !out || !env_desc) return POMCP_E_INVALID;
  *out = nullptr;
  // (the other environments' descriptions have their place in the config: pomcp_create)
  if (cfg->env_id != POMCP_ENV_COOPERATIVE_REACHING && cfg->env_id != POMCP_ENV_PREDATOR_PREY)
    return POMCP_E_UNSUPPORTED;
  const int64_t want = cfg->env_id == POMCP_ENV_PREDATOR_PREY ? (int64_t)sizeof(pomcp_pp_grid)
                                                              : (int64_t)sizeof(pomcp_cr_grid);
  if (env_desc_bytes != want) return POMCP_E_INVALID;
  return create_ctx(cfg, env_desc, device, hip_stream, out);
}

static int create_ctx(const pomcp_config* cfg, const void* desc, int32_t device, void* hip_stream,
                      pomcp_ctx** out) {
  if (!cfg || !out) return POMCP_E_INVALID;
  *out = nullptr;
  std::string why;
  int rc = validate(cfg, desc, &why);
  if (rc != POMCP_OK) {
    std::fprintf(stderr, "pomcp_create: %s\n", why.c_str());
    return rc;
  }
  auto* ctx = new pomcp_ctx();
  ctx->cfg = *cfg;
  if ((rc = ctx->open(device, hip_stream)) != POMCP_OK) {
    delete ctx;
    return rc;
  }
  const pomcp_config& c = *cfg;
  ctx->set_env_model(c, desc);
  DevParams& d = ctx->dp;
  d.env = c.env_id;
  d.B = c.num_trees;
  d.A = c.num_actions;
  d.ego = c.ego_agent;
  d.other = 1 - c.ego_agent;
  d.sel = c.action_selection;
  d.depth_limit = c.depth_limit;
  d.step_limit = c.step_limit;
  d.n_target = c.num_particles + c.extra_particles;
  d.has_kb = c.has_known_bounds;
  d.ncells = (c.grid.obs_front + c.grid.obs_back + 1) * (2 * c.grid.obs_side + 1);
  d.discount = c.discount;
  d.c = c.c;
  d.pucb_f = c.pucb_exploration_fraction;
  d.limit_factor = c.reinvigoration_sample_limit_factor;
  d.kb_min = c.known_min;
  d.kb_max = c.known_max;
  d.Nb = c.max_blocks;
  d.Np = c.max_particles;
  d.Nr = c.max_belief;
  d.H = c.overflow_slots;
  d.bucket_mask = (uint32_t)(c.overflow_slots / kBucket - 1);
  d.ovf_base = (uint32_t)(c.max_blocks * c.num_actions * kSlots + 1);
  d.cut_base = d.ovf_base + (uint32_t)c.overflow_slots;
  d.defer = 1;   // deferred cut-off records (pomcp_set_defer_cutoff)
  d.sel_margin = 1e-12;   // fast-selection margin (pomcp_debug_set_select_margin)
  d.islots = kSlots;
  d.tm = c.type_based;
  d.lines = blk_lines(d.A, d.tm);
  const int64_t B = c.num_trees;
  // (the first failure skips the rest)
  auto alloc = [&](auto*& field, int64_t count) {
    if (rc == POMCP_OK) rc = ctx->alloc(field, (size_t)count);
  };
  alloc(d.hdr, B);
  alloc(d.an, arena_lines((int)B, d.Nb, d.lines));   // interleaved by search wave
  alloc(d.ovf, B * d.H);
  // pomcp_device.h WaveLog: 3 u32 arrays per search wave (+ aux when type-based)
  if (rc == POMCP_OK)
    rc = ctx->alloc_bytes(d.plog, sizeof(uint32_t) * (size_t)((int64_t)search_waves((int)B) * kWave *
                                                              d.Np * (3 + d.tm)));
  if (d.tm && rc == POMCP_OK) rc = ctx->alloc_bytes(d.tmt, sizeof(TmDev));   // tables + ego kinds
  alloc(d.wlog, search_waves((int)B));
  alloc(d.want, B);
  alloc(d.want_info, B);
  alloc(d.cnt, B);
  alloc(d.belief, B * d.Nr);
  alloc(d.path, B * 3 * kMaxPath);
  alloc(d.logtab, c.log_table_size);
  alloc(d.dpow, c.discount_pow_size);
  if (rc == POMCP_OK) rc = ctx->alloc_bytes(d.model, ctx->model_bytes);
  alloc(d.stats, B);
  alloc(d.merge, B * POMCP_XREC(d.A));
  alloc(d.upd_out, B * 2);
  alloc(d.in_actions, B);
  alloc(d.in_obs, B);
  alloc(d.out_obs, B);
  alloc(ctx->merged, B);
  if (rc != POMCP_OK) {
    pomcp_destroy(ctx);
    return rc;
  }
  d.logtab_n = c.log_table_size;
  d.dpow_n = (int32_t)(c.discount_pow_size > INT32_MAX ? INT32_MAX : c.discount_pow_size);
  hipStream_t s = ctx->stream;
  // zero: hash epoch 0 is never valid, headers start empty
  if (hipMemsetAsync(d.ovf, 0, sizeof(OvfSlot) * (size_t)(B * d.H), s) != hipSuccess ||
      hipMemsetAsync(d.hdr, 0, sizeof(TreeHdr) * (size_t)B, s) != hipSuccess ||
      hipMemsetAsync(d.stats, 0, sizeof(pomcp_root_stats) * (size_t)B, s) != hipSuccess ||
      ctx->upload(d.logtab, c.log_table, (size_t)c.log_table_size) != POMCP_OK ||
      ctx->upload(d.dpow, c.discount_pow, (size_t)c.discount_pow_size) != POMCP_OK ||
      ctx->upload_bytes(d.model, ctx->host_model, ctx->model_bytes) != POMCP_OK) {
    ctx->err = "initial upload failed";
    pomcp_destroy(ctx);
    return POMCP_E_HIP;
  }
  // headers: keys and counters
  std::vector<TreeHdr> h((size_t)B);
  for (int64_t t = 0; t < B; ++t) {
    std::memset(&h[t], 0, sizeof(TreeHdr));
    h[t].seed = c.seed;
    h[t].tree_key = c.tree_key_base + (uint32_t)t;
  }
  // same stream as the zeroing memset above (the engine stream is non-blocking:
  // a null-stream copy would not be ordered after it)
  if (ctx->upload(d.hdr, h.data(), (size_t)B) != POMCP_OK) {
    ctx->err = "header upload failed";
    pomcp_destroy(ctx);
    return POMCP_E_HIP;
  }
  ctx->host_upd.resize((size_t)(2 * B));
  ctx->host_stats.resize((size_t)B);
  // tables and headers were copied asynchronously from caller / local memory:
  // finish before returning
  if (hipStreamSynchronize(s) != hipSuccess) {
    pomcp_destroy(ctx);
    return POMCP_E_HIP;
  }
  rc = pomcp_reset(ctx);
  if (rc != POMCP_OK) {
    pomcp_destroy(ctx);
    return rc;
  }
  *out = ctx;
  return POMCP_OK;
}

void pomcp_destroy(pomcp_ctx* ctx) {
  if (!ctx) return;
  ctx->close();
  if (ctx->snap_hdr) (void)hipFree(ctx->snap_hdr);
  ctx->destroy_events();
  for (hipEvent_t e : ctx->acc_ev)
    if (e) (void)hipEventDestroy(e);
  delete ctx;
}

int pomcp_reset(pomcp_ctx* ctx) {
  if (!ctx) return POMCP_E_INVALID;
  PB_TRY(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_reset, dim3(grid_blocks(ctx->dp.B)), dim3(256), 0, ctx->stream, ctx->dp);
  PB_TRY(ctx, hipGetLastError());
  ctx->have_snapshot = false;
  ctx->defer_pending = false;
  ctx->have_root = false;
  ctx->ep_active = false;   // a batch of episodes ends with its trees
  ctx->q_active = false;    // and its queue
  ctx->gq_active = false;
  return POMCP_OK;
}

static int first_update_error(pomcp_ctx* ctx) {   // host_upd: [B][2] {root_abs, error}
  return first_tree_error(ctx, "update", [&](int t) { return ctx->host_upd[2 * (size_t)t + 1]; });
}

// Scratch of the subtree compaction (k_compact), allocated on the first
// re-root: a batch that is only ever searched from its initial update (the
// bench's restore loop) never pays for it.
static int ensure_compaction_scratch(pomcp_ctx* ctx) {
  DevParams& d = ctx->dp;
  if (d.cmap) return POMCP_OK;
  const int64_t B = d.B;
  // the streaming scan's look-back records: every wave log's capacity in
  // segments; zeroed (tag epoch 0 is never current)
  const int waves = search_waves((int)B);
  d.lf_nseg = (int32_t)((kWave * d.Np + kLfSeg - 1) / kLfSeg);
  const size_t nd = (size_t)waves * (size_t)((d.lf_nseg + kLfChunk - 1) / kLfChunk);
  int rc;
  if ((rc = ctx->alloc(d.cmap, (size_t)(B * d.Nb))) != POMCP_OK ||
      (rc = ctx->alloc(d.cpar, (size_t)(B * d.Nb))) != POMCP_OK ||
      (rc = ctx->alloc(d.ovf_new, (size_t)(B * d.H))) != POMCP_OK ||
      (rc = ctx->alloc(d.ovf_tmp, (size_t)(B * d.H))) != POMCP_OK ||
      (rc = ctx->alloc(d.scan_info, (size_t)B)) != POMCP_OK ||
      (rc = ctx->alloc(d.lf_desc, nd)) != POMCP_OK ||
      (rc = ctx->alloc(d.lf_fail, 2)) != POMCP_OK ||
      (rc = ctx->alloc(d.cm16, (size_t)waves * kCm16)) != POMCP_OK ||
      (rc = ctx->alloc(d.cm16_off, (size_t)waves * kCm16Off)) != POMCP_OK)
    return rc;
  PB_TRY(ctx, hipMemsetAsync(d.lf_desc, 0, sizeof(LfDesc) * nd, ctx->stream));
  ctx->lf_epoch = 0;
  const char* ls = std::getenv("POMCP_LOG_SCAN");
  ctx->log_scan_legacy = ls != nullptr && std::string(ls) == "legacy";
  // tests only: the filter classifies from the global block maps (the path of
  // logs whose 64 trees' maps do not fit the packed table)
  const char* pk = std::getenv("POMCP_LF_PACKED_CMAP");
  ctx->lf_packed_cmap = !(pk != nullptr && std::string(pk) == "off");
  // the persistent grid: as many workgroups as are resident at once
  int per_cu = 0, ncu = 0;
  PB_TRY(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(
                  &per_cu, reinterpret_cast<const void*>(
                               d.env == POMCP_ENV_PREDATOR_PREY        ? &k_log_filter<EnvPredatorPrey>
                               : d.env == POMCP_ENV_COOPERATIVE_REACHING ? &k_log_filter<EnvCoopReaching>
                               : d.env == POMCP_ENV_PURSUIT_EVASION    ? &k_log_filter<EnvPursuitEvasion>
                                                                       : &k_log_filter<EnvDriving>),
                  kLfThreads, 0));
  PB_TRY(ctx, hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, ctx->device));
  ctx->lf_grid = (per_cu > 0 ? per_cu : 1) * (ncu > 0 ? ncu : 1);
  return POMCP_OK;
}

// The update's launches on inputs already in dp.in_actions / dp.in_obs
// (pomcp_update uploads them; a batched episode step leaves them there).
// reroot: some tree has an action (it is not the batch's initial update).
// Asynchronous: the caller reads dp.upd_out / dp.lf_fail and synchronises.
static int launch_update(pomcp_ctx* ctx, bool reroot) {
  const int B = ctx->dp.B;
  // re-root: child lookup per tree; subtree compaction to the child's subtree
  // (re-roots only: an initial update leaves an empty arena) with one ordered
  // scan of each search wave's log that also extracts the child's particles;
  // then the per-tree update (initial belief / new root + reinvigoration)
  with_env(ctx, [&](auto e) {
    hipLaunchKernelGGL(k_reroot_child<decltype(e)>, dim3(grid_blocks(B)), dim3(256), 0, ctx->stream,
                       ctx->dp);
  });
  PB_TRY(ctx, hipGetLastError());
  if (reroot) {
    int rc = ensure_compaction_scratch(ctx);
    if (rc != POMCP_OK) return rc;
    hipLaunchKernelGGL(k_compact, dim3(grid_blocks(B)), dim3(256), 0, ctx->stream, ctx->dp);
    PB_TRY(ctx, hipGetLastError());
    if (ctx->log_scan_legacy) {
      with_env(ctx, [&](auto e) {
        hipLaunchKernelGGL(k_compact_log<decltype(e)>, dim3((unsigned)search_waves(B)),
                           dim3(64 * kLogWaves), 0, ctx->stream, ctx->dp);
      });
    } else {
      // the streaming scan: the filter over every log's segments, then the
      // materialising pass over the kept records
      if (++ctx->lf_epoch >= (1u << 30)) {   // (tags hold 30 bits: start over on zeroed records)
        PB_TRY(ctx, hipMemsetAsync(ctx->dp.lf_desc, 0,
                                   sizeof(LfDesc) * (size_t)search_waves(B) *
                                       (size_t)((ctx->dp.lf_nseg + kLfChunk - 1) / kLfChunk),
                                   ctx->stream));
        ctx->lf_epoch = 1;
      }
      ctx->dp.lf_epoch = ctx->lf_epoch;
      PB_TRY(ctx, hipMemsetAsync(ctx->dp.lf_fail, 0, 2 * sizeof(uint32_t), ctx->stream));
      hipLaunchKernelGGL(k_pack_cmap, dim3((unsigned)search_waves(B)), dim3(256), 0, ctx->stream, ctx->dp,
                         ctx->lf_packed_cmap ? 1 : 0);
      PB_TRY(ctx, hipGetLastError());
      with_env(ctx, [&](auto e) {
        hipLaunchKernelGGL(k_log_filter<decltype(e)>, dim3((unsigned)ctx->lf_grid), dim3(kLfThreads), 0,
                           ctx->stream, ctx->dp, search_waves(B));
      });
      PB_TRY(ctx, hipGetLastError());
      with_env(ctx, [&](auto e) {
        hipLaunchKernelGGL((k_compact_log<decltype(e), true>), dim3((unsigned)search_waves(B)),
                           dim3(64 * kMatWaves), 0, ctx->stream, ctx->dp);
      });
    }
    PB_TRY(ctx, hipGetLastError());
  }
  with_env(ctx, [&](auto e) {
    hipLaunchKernelGGL(k_update<decltype(e)>, dim3(grid_blocks(B)), dim3(256), 0, ctx->stream, ctx->dp);
  });
  PB_TRY(ctx, hipGetLastError());
  return POMCP_OK;
}

int pomcp_update(pomcp_ctx* ctx, const int32_t* actions, const uint64_t* obs_keys,
                 int32_t* root_absorbing_out) {
  if (!ctx || !obs_keys) return POMCP_E_INVALID;
  if (ctx->dp.tm && !ctx->tm_set) return fail(ctx, POMCP_E_STATE, "update: pomcp_set_type_policies first");
  PB_TRY(ctx, hipSetDevice(ctx->device));
  const int B = ctx->dp.B;
  std::vector<int32_t> acts((size_t)B, -1);
  if (actions) std::memcpy(acts.data(), actions, sizeof(int32_t) * (size_t)B);
  int rc;
  if ((rc = ctx->upload(ctx->dp.in_actions, acts.data(), (size_t)B)) != POMCP_OK ||
      (rc = ctx->upload(ctx->dp.in_obs, obs_keys, (size_t)B)) != POMCP_OK)
    return rc;
  bool reroot = false;
  for (int t = 0; t < B && !reroot; ++t) reroot = acts[t] >= 0;
  if ((rc = launch_update(ctx, reroot)) != POMCP_OK) return rc;
  PB_TRY(ctx, hipMemcpyAsync(ctx->host_upd.data(), ctx->dp.upd_out, sizeof(int32_t) * 2 * B,
                             hipMemcpyDeviceToHost, ctx->stream));
  uint32_t lf_fail = 0u;
  if (reroot && !ctx->log_scan_legacy)
    PB_TRY(ctx, hipMemcpyAsync(&lf_fail, ctx->dp.lf_fail, sizeof(uint32_t), hipMemcpyDeviceToHost,
                               ctx->stream));
  PB_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (lf_fail != 0u) return fail(ctx, POMCP_E_HIP, "update: the log scan's look-back gave up");
  ctx->defer_pending = false;   // k_compact_log materialised the surviving deferred children
  ctx->have_root = true;
  if (root_absorbing_out)
    for (int t = 0; t < B; ++t) root_absorbing_out[t] = ctx->host_upd[2 * t];
  return first_update_error(ctx);
}

// (CooperativeReaching-v0 and PredatorPrey-v0 run the tree-per-lane kernel only)
static bool lane_only_env(int32_t env) {
  return env == POMCP_ENV_COOPERATIVE_REACHING || env == POMCP_ENV_PREDATOR_PREY;
}
static bool wave_search_fits(const pomcp_ctx* ctx) {
  return !lane_only_env(ctx->dp.env) && ctx->dp.A <= kMaxA &&
         (int64_t)ctx->dp.B * ctx->dp.Np * (int64_t)sizeof(LogRec) <= kWaveSearchMaxScratch;
}

static int resolve_search_kind(const pomcp_ctx* ctx) {
  if (ctx->dp.tm) return POMCP_SEARCH_LANE;   // the type-based search is k_search<..., TM = 1>
  if (ctx->search_kind == POMCP_SEARCH_WAVE) return POMCP_SEARCH_WAVE;
  if (ctx->search_kind == POMCP_SEARCH_LANE) return POMCP_SEARCH_LANE;
  return ctx->dp.B <= kWaveSearchMaxTrees && wave_search_fits(ctx) ? POMCP_SEARCH_WAVE
                                                                   : POMCP_SEARCH_LANE;
}

int pomcp_set_search_kernel(pomcp_ctx* ctx, int32_t kind) {
  if (!ctx || kind < POMCP_SEARCH_AUTO || kind > POMCP_SEARCH_WAVE) return POMCP_E_INVALID;
  if (kind == POMCP_SEARCH_WAVE && lane_only_env(ctx->dp.env))
    return fail(ctx, POMCP_E_UNSUPPORTED,
                ctx->dp.env == POMCP_ENV_PREDATOR_PREY
                    ? "set_search_kernel: PredatorPrey-v0 has no wave-per-tree search"
                    : "set_search_kernel: CooperativeReaching-v0 has no wave-per-tree search");
  if (kind == POMCP_SEARCH_WAVE && !wave_search_fits(ctx))
    return fail(ctx, POMCP_E_UNSUPPORTED, "set_search_kernel: wave search scratch too large");
  if (kind == POMCP_SEARCH_WAVE && ctx->dp.tm)
    return fail(ctx, POMCP_E_UNSUPPORTED, "set_search_kernel: the type-based search is lane-per-tree");
  if (ctx->defer_pending) {
    const int was = ctx->search_kind;
    ctx->search_kind = kind;
    const bool same = resolve_search_kind(ctx) == POMCP_SEARCH_LANE;
    ctx->search_kind = was;
    if (!same)
      return fail(ctx, POMCP_E_STATE, "set_search_kernel: deferred cut-off records are pending "
                                      "(update, reset or restore first)");
  }
  ctx->search_kind = kind;
  return POMCP_OK;
}

int32_t pomcp_search_kernel_used(const pomcp_ctx* ctx) {
  return ctx ? resolve_search_kind(ctx) : POMCP_E_INVALID;
}

int pomcp_set_defer_cutoff(pomcp_ctx* ctx, int32_t on) {
  if (!ctx || (on != 0 && on != 1)) return POMCP_E_INVALID;
  if (ctx->defer_pending && on != ctx->dp.defer)
    return fail(ctx, POMCP_E_STATE, "set_defer_cutoff: deferred cut-off records are pending "
                                    "(update, reset or restore first)");
  ctx->dp.defer = on;
  return POMCP_OK;
}

// The wave search with step-tree producer waves (pomcp_search_lds.hip) when
// simulations are short enough that the producers' prediction of their draws
// (depth_limit + 1 words per simulation) mostly holds and the first three
// levels are most of a simulation; POMCP_STEP_TREE=0/1 forces it off / on.
static bool use_step_tree(const pomcp_ctx* ctx) {
  const char* f = std::getenv("POMCP_STEP_TREE");
  if (f != nullptr && f[0] != '\0') return f[0] != '0';
  return ctx->dp.depth_limit <= kStepTreeMaxDepth;
}

static int launch_search_wave(pomcp_ctx* ctx, int32_t num_sims, int final_sel) {
  if (!ctx->dp.lscr) {   // the per-tree scratch log, on first use
    const int rc = ctx->alloc(ctx->dp.lscr, (size_t)ctx->dp.B * (size_t)ctx->dp.Np);
    if (rc != POMCP_OK) return rc;
  }
  using KFn = void (*)(DevParams, int, int);
#define PB_LDS_ROW(NP)                                                                          \
  {{k_search_lds<EnvDriving, POMCP_SEL_PUCB, 5, NP>, k_search_lds<EnvDriving, POMCP_SEL_UCB, 5, NP>, \
    k_search_lds<EnvDriving, POMCP_SEL_UNIFORM, 5, NP>},                                         \
   {k_search_lds<EnvPursuitEvasion, POMCP_SEL_PUCB, 4, NP>,                                      \
    k_search_lds<EnvPursuitEvasion, POMCP_SEL_UCB, 4, NP>,                                       \
    k_search_lds<EnvPursuitEvasion, POMCP_SEL_UNIFORM, 4, NP>}}
  static const KFn table[2][2][3] = {PB_LDS_ROW(0), PB_LDS_ROW(kSpecProducers)};
#undef PB_LDS_ROW
  const int e = ctx->dp.env == POMCP_ENV_PURSUIT_EVASION ? 1 : 0;
  const int spec = use_step_tree(ctx) ? 1 : 0;
  hipLaunchKernelGGL(table[spec][e][ctx->dp.sel], dim3((unsigned)ctx->dp.B),
                     dim3((unsigned)(kWave * (1 + spec * kSpecProducers))), 0, ctx->stream, ctx->dp,
                     (int)num_sims, final_sel);
  PB_TRY(ctx, hipGetLastError());
  const int nsw = search_waves(ctx->dp.B);
  hipLaunchKernelGGL(k_log_merge, dim3((unsigned)(ctx->dp.B < kWave ? ctx->dp.B : kWave), (unsigned)nsw),
                     dim3(256), 0, ctx->stream, ctx->dp);
  PB_TRY(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_log_merge_end, dim3((unsigned)((nsw + 63) / 64)), dim3(64), 0, ctx->stream,
                     ctx->dp, nsw);
  PB_TRY(ctx, hipGetLastError());
  return POMCP_OK;
}

// The compile-time depth limit of the tree-per-lane kernel a launch uses
// (k_search's DL, pomcp_search.hip): the context's own when a specialised
// kernel exists for it, else 0, the generic kernel; POMCP_SEARCH_DEPTH_SPEC=0
// forces the generic one (A/B runs and tests; results are the same).
static int search_depth_spec(const pomcp_ctx* ctx) {
  const char* f = std::getenv("POMCP_SEARCH_DEPTH_SPEC");
  if (f != nullptr && f[0] == '0') return 0;
  if (ctx->dp.tm || ctx->dp.depth_limit < 1 || ctx->dp.depth_limit > kRegPath) return 0;
  return ctx->dp.depth_limit;
}

int pomcp_debug_search_depth_spec(const pomcp_ctx* ctx) {
  if (!ctx) return POMCP_E_INVALID;
  return resolve_search_kind(ctx) == POMCP_SEARCH_WAVE ? 0 : search_depth_spec(ctx);
}

static int launch_search(pomcp_ctx* ctx, int32_t num_sims, int final_sel) {
  if (!ctx || num_sims < 0) return POMCP_E_INVALID;
  if (ctx->dp.tm && !ctx->tm_set) return fail(ctx, POMCP_E_STATE, "search: pomcp_set_type_policies first");
  PB_TRY(ctx, hipSetDevice(ctx->device));
  if (resolve_search_kind(ctx) == POMCP_SEARCH_WAVE) return launch_search_wave(ctx, num_sims, final_sel);
  const int tpb = search_tpb(ctx->dp.B);
  const dim3 grid((unsigned)((ctx->dp.B + tpb - 1) / tpb)), block((unsigned)tpb);
  // kernel per (environment, selection rule, workgroup size); the action count is the model's
  const int e = env_row(ctx->dp.env);
  const int row = (ctx->dp.tm ? 2 : 0) + (tpb == kTPB ? 0 : 1);
  int sims = (int)num_sims, fsel = final_sel;
  void* args[] = {&ctx->dp, &sims, &fsel};
  const int dl = search_depth_spec(ctx);
  PB_TRY(ctx, hipLaunchKernel(pb_search_kernel(row, e, ctx->dp.sel, dl), grid, block, args, 0, ctx->stream));
  PB_TRY(ctx, hipGetLastError());
  if (ctx->dp.defer && !ctx->dp.tm && num_sims > 0) ctx->defer_pending = true;
  return POMCP_OK;
}

int pomcp_search(pomcp_ctx* ctx, int32_t num_sims, int32_t* actions_out) {
  int rc = launch_search(ctx, num_sims, 1);
  if (rc != POMCP_OK || !actions_out) return rc;
  rc = pomcp_get_root_stats(ctx, ctx->host_stats.data());
  if (rc != POMCP_OK) return rc;
  for (int t = 0; t < ctx->dp.B; ++t) actions_out[t] = ctx->host_stats[t].action;
  return POMCP_OK;
}

int pomcp_search_continue(pomcp_ctx* ctx, int32_t num_sims) { return launch_search(ctx, num_sims, 0); }

int pomcp_get_root_stats(pomcp_ctx* ctx, pomcp_root_stats* out) {
  if (!ctx || !out) return POMCP_E_INVALID;
  PB_TRY(ctx, hipSetDevice(ctx->device));
  const int rc = ctx->fetch(out, ctx->dp.stats, (size_t)ctx->dp.B);
  if (rc != POMCP_OK) return rc;
  return first_tree_error(ctx, "search", [&](int t) { return out[t].error; });
}

// One tree's header, from the device.
static int fetch_hdr(pomcp_ctx* ctx, int32_t tree, TreeHdr* h) {
  PB_TRY(ctx, hipSetDevice(ctx->device));
  return ctx->fetch(h, ctx->dp.hdr + tree, 1);
}

int pomcp_set_root_belief(pomcp_ctx* ctx, int32_t tree, const uint32_t* particles, int32_t count) {
  if (!ctx || tree < 0 || tree >= ctx->dp.B || count < 1 || !particles)
    return fail(ctx, POMCP_E_INVALID, "set_root_belief: bad arguments");
  if (ctx->dp.tm)
    return fail(ctx, POMCP_E_UNSUPPORTED, "set_root_belief: type-based particles carry a policy");
  if (count > ctx->dp.Nr / 2)   // (the next belief needs room too: half the region)
    return fail(ctx, POMCP_E_ARENA, "set_root_belief: more particles than max_belief / 2");
  const uint32_t t = particles[0];
  for (int32_t i = 0; i < count; ++i)
    if (particles[3 * i] != t || t < 1u)
      return fail(ctx, POMCP_E_INVALID, "set_root_belief: every particle needs the same t >= 1");
  TreeHdr h;
  int rc = fetch_hdr(ctx, tree, &h);
  if (rc != POMCP_OK) return rc;
  if (h.root_t != 0 || h.n_blocks != 0 || h.error != 0)
    return fail(ctx, POMCP_E_STATE, "set_root_belief: the tree must be fresh (pomcp_reset)");
  // the region's records [at, at + count) in memory order (bel_at: the end of
  // the region, reversed, when the belief grows from there)
  const int sel = h.belief_sel ^ 1;
  const int64_t at = sel ? ctx->dp.Nr - count : 0;
  std::vector<uint4> b((size_t)count);
  for (int32_t i = 0; i < count; ++i)
    b[bel_at(sel, ctx->dp.Nr, i) - at] =
        make_uint4(particles[3 * i], particles[3 * i + 1], particles[3 * i + 2], 0u);
  rc = ctx->upload(ctx->dp.belief + (int64_t)tree * ctx->dp.Nr + at, b.data(), (size_t)count);
  if (rc != POMCP_OK) return rc;
  h.belief_sel = sel;
  h.belief_size = count;
  h.root_t = (int32_t)t;
  h.root_id = kRootId;
  h.root_blk = -1;
  h.root_visits = 0;
  h.root_abs = 0;
  h.n_nodes += 1;
  if ((rc = ctx->upload(ctx->dp.hdr + tree, &h, 1)) != POMCP_OK) return rc;
  PB_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->have_root = true;
  return POMCP_OK;
}

// The first n particles of a tree's root belief, in order (pomcp_device.h
// bel_at: a belief grown from the region's end is stored reversed)
static int read_root_belief(pomcp_ctx* ctx, int32_t tree, const TreeHdr& h, int n, uint4* out) {
  const int sel = h.belief_sel;
  const int64_t at = sel ? ctx->dp.Nr - n : 0;
  std::vector<uint4> raw((size_t)n);
  const int rc = ctx->fetch(raw.data(), ctx->dp.belief + (int64_t)tree * ctx->dp.Nr + at, (size_t)n);
  if (rc != POMCP_OK) return rc;
  for (int i = 0; i < n; ++i) out[i] = raw[bel_at(sel, ctx->dp.Nr, i) - at];
  return POMCP_OK;
}

int pomcp_get_root_belief(pomcp_ctx* ctx, int32_t tree, uint32_t* out, int32_t capacity,
                          int32_t* count) {
  if (!ctx || !count || tree < 0 || tree >= ctx->dp.B) return POMCP_E_INVALID;
  TreeHdr h;
  int rc = fetch_hdr(ctx, tree, &h);
  if (rc != POMCP_OK) return rc;
  *count = h.belief_size;
  if (!out || capacity <= 0) return POMCP_OK;
  const int n = h.belief_size < capacity ? h.belief_size : capacity;
  std::vector<uint4> tmp((size_t)n);
  if ((rc = read_root_belief(ctx, tree, h, n, tmp.data())) != POMCP_OK) return rc;
  for (int i = 0; i < n; ++i) {
    out[3 * i + 0] = tmp[i].x;
    out[3 * i + 1] = tmp[i].y;
    out[3 * i + 2] = tmp[i].z;
  }
  return POMCP_OK;
}

// The context's tables and ego kinds to p.tmt's TmDev, complete on return.
static int upload_tm(pomcp_ctx* ctx) {
  TmDev dev;
  dev.t = ctx->host_tm;
  dev.e = ctx->host_tme;
  const int rc = ctx->upload_bytes(ctx->dp.tmt, &dev, sizeof(dev));
  if (rc != POMCP_OK) return rc;
  PB_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return POMCP_OK;
}

int pomcp_set_type_policies(pomcp_ctx* ctx, const pomcp_type_policies* tp) {
  if (!ctx || !tp) return POMCP_E_INVALID;
  if (!ctx->dp.tm) return fail(ctx, POMCP_E_STATE, "set_type_policies: context is not type_based");
  const int A = ctx->dp.A, ne = tp->num_ego, no = tp->num_other;
  if (ne < 1 || ne > kTmMax || no < 1 || no > kTmMax)
    return fail(ctx, POMCP_E_INVALID, "set_type_policies: 1..8 ego and other-agent policies");
  TmTables t{};
  t.n_ego = ne;
  t.n_other = no;
  t.no_meta_draw = tp->no_meta_draw != 0;
  t.no_mixture_draw = tp->no_mixture_draw != 0;
  t.ego_uniform = tp->ego_uniform != 0;
  t.other_uniform = tp->other_uniform != 0;
  if (t.no_mixture_draw && no != 1)
    return fail(ctx, POMCP_E_INVALID, "set_type_policies: no_mixture_draw needs one other-agent policy");
  // random.choices' cumulative weights (itertools.accumulate) and total = cum[-1] + 0.0
  auto cum = [](const double* w, int n, double* c, double* total) {
    double acc = 0.0;
    for (int i = 0; i < n; ++i) {
      acc = i == 0 ? w[i] : acc + w[i];
      c[i] = acc;
    }
    *total = acc + 0.0;
  };
  for (int a = 0; a < A; ++a) t.prior[0][a] = tp->expected_prior[a];
  for (int k = 0; k < ne; ++k) {
    for (int a = 0; a < A; ++a) {
      if (!(tp->ego_pi[k][a] >= 0.0)) return fail(ctx, POMCP_E_INVALID, "set_type_policies: ego_pi < 0");
      t.prior[k + 1][a] = tp->ego_pi[k][a];
    }
    cum(tp->ego_pi[k], A, t.ego_cum[k], &t.ego_tot[k]);
    if (!(t.ego_tot[k] > 0.0)) return fail(ctx, POMCP_E_INVALID, "set_type_policies: ego_pi sums to 0");
  }
  for (int j = 0; j < no; ++j) {
    for (int a = 0; a < A; ++a)
      if (!(tp->other_pi[j][a] >= 0.0)) return fail(ctx, POMCP_E_INVALID, "set_type_policies: other_pi < 0");
    cum(tp->other_pi[j], A, t.oth_cum[j], &t.oth_tot[j]);
    if (!(t.oth_tot[j] > 0.0)) return fail(ctx, POMCP_E_INVALID, "set_type_policies: other_pi sums to 0");
    const int m = tp->meta_len[j];
    if (m < 1 || m > kTmMax) return fail(ctx, POMCP_E_INVALID, "set_type_policies: meta_len 1..8");
    t.meta_len[j] = m;
    for (int i = 0; i < m; ++i) {
      const int k = tp->meta_policy[j][i];
      if (k < 0 || k >= ne) return fail(ctx, POMCP_E_INVALID, "set_type_policies: meta_policy index");
      t.meta_idx[j][i] = k;
    }
    cum(tp->meta_weight[j], m, t.meta_cum[j], &t.meta_tot[j]);
  }
  PB_TRY(ctx, hipSetDevice(ctx->device));
  ctx->host_tm = t;
  std::memset(ctx->host_other_pi, 0, sizeof(ctx->host_other_pi));
  for (int j = 0; j < no; ++j)
    for (int a = 0; a < A; ++a) ctx->host_other_pi[j][a] = tp->other_pi[j][a];
  ctx->host_tme = TmEgo{};   // every ego policy fixed (pomcp_set_type_ego_kinds)
  const int rc = upload_tm(ctx);
  if (rc != POMCP_OK) return rc;
  ctx->tm_set = true;
  return POMCP_OK;
}

int pomcp_set_type_policy_kinds(pomcp_ctx* ctx, const pomcp_policy_kinds* kinds) {
  if (!ctx) return POMCP_E_INVALID;
  if (!ctx->dp.tm || !ctx->tm_set)
    return fail(ctx, POMCP_E_STATE, "set_type_policy_kinds: pomcp_set_type_policies first");
  TmTables t = ctx->host_tm;
  for (int j = 0; j < kTmMax; ++j) t.oth_kind[j] = t.oth_p0[j] = t.oth_p1[j] = 0;
  for (int j = 0; kinds && j < t.n_other; ++j) {
    if (!policy_kind_ok(kinds->kind[j], kinds->param0[j], kinds->param1[j]))
      return fail(ctx, POMCP_E_INVALID, "set_type_policy_kinds: kind 1 (caution 0..15, vmax 0..3), "
                                        "kind 3 (rule 0..4, 0), kind 5 (rule 0..2, 0) or 0");
    if (kinds->kind[j] == POMCP_POLICY_FIXED) continue;
    bool has = false;
    with_episode_env(ctx, [&](auto e) { has = decltype(e)::has_kind(kinds->kind[j]); });
    if (!has)
      return fail(ctx, POMCP_E_UNSUPPORTED, "set_type_policy_kinds: the environment has no such "
                                            "reactive policy kind");
    if (t.other_uniform)
      return fail(ctx, POMCP_E_INVALID, "set_type_policy_kinds: other_uniform draws no policy");
    t.oth_kind[j] = kinds->kind[j];
    t.oth_p0[j] = kinds->param0[j];
    t.oth_p1[j] = kinds->param1[j];
  }
  PB_TRY(ctx, hipSetDevice(ctx->device));
  ctx->host_tm = t;
  return upload_tm(ctx);
}

int pomcp_set_type_ego_kinds(pomcp_ctx* ctx, const pomcp_policy_kinds* kinds,
                             const double* expected_meta) {
  if (!ctx) return POMCP_E_INVALID;
  if (!ctx->dp.tm || !ctx->tm_set)
    return fail(ctx, POMCP_E_STATE, "set_type_ego_kinds: pomcp_set_type_policies first");
  const TmTables& t = ctx->host_tm;
  TmEgo e{};
  for (int k = 0; kinds && k < t.n_ego; ++k) {
    if (!policy_kind_ok(kinds->kind[k], kinds->param0[k], kinds->param1[k]))
      return fail(ctx, POMCP_E_INVALID, "set_type_ego_kinds: kind 3 (rule 0..4, 0) or 0");
    if (kinds->kind[k] == POMCP_POLICY_FIXED) continue;
    // an ego kind needs the state form of the policy to hold at every node
    // (DESIGN.md §22): CooperativeReaching's goal heuristics only
    if (ctx->dp.env != POMCP_ENV_COOPERATIVE_REACHING || kinds->kind[k] != POMCP_POLICY_CR_GOAL)
      return fail(ctx, POMCP_E_UNSUPPORTED, "set_type_ego_kinds: the environment has no such "
                                            "reactive ego policy kind");
    if (t.ego_uniform)
      return fail(ctx, POMCP_E_INVALID, "set_type_ego_kinds: ego_uniform draws no policy");
    e.any = 1;
    e.kind[k] = kinds->kind[k];
    e.p0[k] = kinds->param0[k];
    e.p1[k] = kinds->param1[k];
  }
  if (e.any) {
    if (!expected_meta)
      return fail(ctx, POMCP_E_INVALID, "set_type_ego_kinds: expected_meta is NULL");
    double sum = 0.0;
    for (int k = 0; k < t.n_ego; ++k) {
      if (!(expected_meta[k] >= 0.0) || !(expected_meta[k] <= 1.0 + 1e-9))
        return fail(ctx, POMCP_E_INVALID, "set_type_ego_kinds: expected_meta in [0, 1]");
      e.w[k] = expected_meta[k];
      sum += expected_meta[k];
    }
    if (!(sum > 0.0))
      return fail(ctx, POMCP_E_INVALID, "set_type_ego_kinds: expected_meta sums to 0");
  }
  PB_TRY(ctx, hipSetDevice(ctx->device));
  ctx->host_tme = e;
  return upload_tm(ctx);
}

int pomcp_get_root_prior(pomcp_ctx* ctx, int32_t tree, double* out) {
  if (!ctx || !out || tree < 0 || tree >= ctx->dp.B) return POMCP_E_INVALID;
  if (!ctx->dp.tm) return fail(ctx, POMCP_E_STATE, "get_root_prior: context is not type_based");
  TreeHdr h;
  int rc = fetch_hdr(ctx, tree, &h);
  if (rc != POMCP_OK) return rc;
  const int A = ctx->dp.A;
  if (h.root_blk < 0) {   // no block yet: the prior its code names
    const int code = h.root_code >= 0 && h.root_code <= ctx->host_tm.n_ego ? h.root_code : 0;
    if (ctx->host_tme.any) {
      // a reactive ego policy's line is a function of the root: built from a
      // root particle's ego word as the search will build it (never the
      // placeholder row)
      if (h.belief_size <= 0)
        return fail(ctx, POMCP_E_STATE, "get_root_prior: the root has no particle yet");
      uint4 bp;
      if ((rc = read_root_belief(ctx, tree, h, 1, &bp)) != POMCP_OK) return rc;
      const CrModel& m = *static_cast<const CrModel*>(ctx->host_model);
      const TmEgo& e = ctx->host_tme;
      const uint32_t own = ctx->dp.ego == 0 ? bp.y : bp.z;
      tm_prior_line(ctx->host_tm.prior, e, ctx->host_tm.n_ego, A, code,
                    [&](int k) { return cr_goal_action(m, own, e.p0[k]); }, out);
      return POMCP_OK;
    }
    for (int a = 0; a < A; ++a) out[a] = ctx->host_tm.prior[code][a];
    return POMCP_OK;
  }
  const Line* blk = ctx->dp.an + tree_base_lines(tree, ctx->dp.Nb, ctx->dp.lines) +
                    (int64_t)h.root_blk * blk_stride_lines(ctx->dp.lines);
  const uint4* prior = reinterpret_cast<const uint4*>(blk) + part_prior(A);
  return ctx->fetch(out, reinterpret_cast<const double*>(prior), (size_t)A);
}

int pomcp_get_root_policies(pomcp_ctx* ctx, int32_t tree, int32_t* out, int32_t capacity,
                            int32_t* count) {
  if (!ctx || !count || tree < 0 || tree >= ctx->dp.B) return POMCP_E_INVALID;
  if (!ctx->dp.tm) return fail(ctx, POMCP_E_STATE, "get_root_policies: context is not type_based");
  TreeHdr h;
  int rc = fetch_hdr(ctx, tree, &h);
  if (rc != POMCP_OK) return rc;
  *count = h.belief_size;
  if (!out || capacity <= 0) return POMCP_OK;
  const int n = h.belief_size < capacity ? h.belief_size : capacity;
  std::vector<uint4> tmp((size_t)n);
  if ((rc = read_root_belief(ctx, tree, h, n, tmp.data())) != POMCP_OK) return rc;
  for (int i = 0; i < n; ++i) out[i] = (int32_t)tmp[i].w;
  return POMCP_OK;
}

// The query-state buffer of pomcp_belief_stats and its results, on first use.
static int ensure_belief_buffers(pomcp_ctx* ctx) {
  if (ctx->bel_out) return POMCP_OK;
  const int rc = ctx->alloc(ctx->bel_out, (size_t)ctx->dp.B);
  return rc != POMCP_OK ? rc : ctx->alloc(ctx->bel_q, (size_t)ctx->dp.B);
}

// k_belief_stats on the context stream (belief_stats.hip): one workgroup per
// tree, grid-strided beyond kBelMaxGrid; the query states are uploaded first
// when given (upload = false: they are there already).  The results stay in
// ctx->bel_out.
static int launch_belief_stats(pomcp_ctx* ctx, const uint32_t* states, bool upload = true) {
  const int B = ctx->dp.B;
  int rc = ensure_belief_buffers(ctx);
  if (rc != POMCP_OK) return rc;
  if (states && upload &&
      (rc = ctx->upload(ctx->bel_q, reinterpret_cast<const uint2*>(states), (size_t)B)) != POMCP_OK)
    return rc;
  const int num_other = ctx->dp.tm ? ctx->host_tm.n_other : 0;
  hipLaunchKernelGGL(k_belief_stats, dim3((unsigned)(B < kBelMaxGrid ? B : kBelMaxGrid)),
                     dim3(kBelThreads), 0, ctx->stream, ctx->dp,
                     states ? (const uint2*)ctx->bel_q : (const uint2*)nullptr, num_other,
                     ctx->bel_out);
  PB_TRY(ctx, hipGetLastError());
  return POMCP_OK;
}

static int belief_stats_ready(pomcp_ctx* ctx) {
  if (ctx->dp.tm && !ctx->tm_set)
    return fail(ctx, POMCP_E_STATE, "belief_stats: pomcp_set_type_policies first");
  if (!ctx->have_root)
    return fail(ctx, POMCP_E_STATE, "belief_stats: no root belief yet (update first)");
  return POMCP_OK;
}

int pomcp_belief_stats(pomcp_ctx* ctx, const uint32_t* states, pomcp_belief_counts* out) {
  if (!ctx || !out) return fail(ctx, POMCP_E_INVALID, "belief_stats: null argument");
  int rc = belief_stats_ready(ctx);
  if (rc != POMCP_OK) return rc;
  PB_TRY(ctx, hipSetDevice(ctx->device));
  rc = launch_belief_stats(ctx, states);
  if (rc != POMCP_OK) return rc;
  if ((rc = ctx->fetch(out, ctx->bel_out, (size_t)ctx->dp.B)) != POMCP_OK) return rc;
  return first_error(ctx, ctx->dp.B, [&](int t) { return out[t].error; }, [](int t, int e) {
    return "belief_stats: tree " + std::to_string(t) + ": error " + std::to_string(e) +
           " (its own, or a particle's policy index out of range)";
  });
}

int pomcp_arena_usage(pomcp_ctx* ctx, int32_t* max_blocks_used, int32_t* max_log_used) {
  if (!ctx || !max_blocks_used || !max_log_used) return POMCP_E_INVALID;
  PB_TRY(ctx, hipSetDevice(ctx->device));
  std::vector<TreeHdr> h((size_t)ctx->dp.B);
  int rc = ctx->fetch(h.data(), ctx->dp.hdr, h.size());
  if (rc != POMCP_OK) return rc;
  int32_t nb = 0, nl = 0;
  for (const auto& x : h) {
    nb = x.n_blocks > nb ? x.n_blocks : nb;
    nl = x.n_log > nl ? x.n_log : nl;
  }
  *max_blocks_used = nb;
  *max_log_used = nl;
  return POMCP_OK;
}

int pomcp_rekey(pomcp_ctx* ctx, uint64_t seed) {
  if (!ctx) return POMCP_E_INVALID;
  PB_TRY(ctx, hipSetDevice(ctx->device));
  std::vector<TreeHdr> h((size_t)ctx->dp.B);
  int rc = ctx->fetch(h.data(), ctx->dp.hdr, h.size());
  if (rc != POMCP_OK) return rc;
  for (auto& x : h) x.seed = seed;
  if ((rc = ctx->upload(ctx->dp.hdr, h.data(), h.size())) != POMCP_OK) return rc;
  PB_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return POMCP_OK;
}

int pomcp_root_merge_buffer(pomcp_ctx* ctx, void** device_ptr) {
  if (!ctx || !device_ptr) return POMCP_E_INVALID;
  *device_ptr = ctx->dp.merge;
  return POMCP_OK;
}

int pomcp_root_gather_buffer(pomcp_ctx* ctx, int32_t world, void** device_ptr) {
  if (!ctx || !device_ptr || world < 1) return POMCP_E_INVALID;
  if (world > ctx->gather_world) {
    PB_TRY(ctx, hipSetDevice(ctx->device));
    PB_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->gather) {
      for (auto& q : ctx->allocs)
        if (q == ctx->gather) q = nullptr;
      (void)hipFree(ctx->gather);
      ctx->gather = nullptr;
      ctx->gather_world = 0;
    }
    const size_t n = (size_t)world * (size_t)ctx->dp.B * POMCP_XREC(ctx->dp.A);
    const int rc = ctx->alloc(ctx->gather, n);
    if (rc != POMCP_OK) return rc;
    PB_TRY(ctx, hipMemsetAsync(ctx->gather, 0, sizeof(double) * n, ctx->stream));
    ctx->gather_world = world;
  }
  *device_ptr = ctx->gather;
  return POMCP_OK;
}

// ncclAllGather of the RCCL copy already in this process (PyTorch's, or one
// the caller loaded; its soname is librccl.so.1): never a second copy, whose
// functions would be handed a communicator created by the first one.
typedef int (*pb_nccl_allgather_fn)(const void*, void*, size_t, int, void*, hipStream_t);
static pb_nccl_allgather_fn pb_rccl_allgather() {
  static pb_nccl_allgather_fn fn = nullptr;
  if (!fn) {
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_NOLOAD);
    if (h) fn = reinterpret_cast<pb_nccl_allgather_fn>(dlsym(h, "ncclAllGather"));
  }
  return fn;
}

int pomcp_allgather_root(pomcp_ctx* ctx, void* rccl_comm, int32_t world) {
  if (!ctx || !rccl_comm || world < 1) return POMCP_E_INVALID;
  PB_TRY(ctx, hipSetDevice(ctx->device));
  const pb_nccl_allgather_fn allgather = pb_rccl_allgather();
  if (!allgather)
    return fail(ctx, POMCP_E_UNSUPPORTED,
                "allgather_root: no RCCL library is loaded in this process (load the one the "
                "communicator was created with first)");
  void* gbuf = nullptr;
  int rc = pomcp_root_gather_buffer(ctx, world, &gbuf);
  if (rc != POMCP_OK) return rc;
  constexpr int kNcclFloat64 = 8;   // rccl.h ncclDataType_t
  const size_t n = (size_t)ctx->dp.B * POMCP_XREC(ctx->dp.A);
  rc = allgather(ctx->dp.merge, gbuf, n, kNcclFloat64, rccl_comm, ctx->stream);
  if (rc != 0) return fail(ctx, POMCP_E_HIP, "allgather_root: ncclAllGather error " + std::to_string(rc));
  return POMCP_OK;
}

int pomcp_merge_roots(pomcp_ctx* ctx, int32_t group, int32_t world, pomcp_merged_root* out) {
  if (!ctx || group < 1 || ctx->dp.B % group != 0)
    return fail(ctx, POMCP_E_INVALID, "merge_roots: group must divide num_trees");
  if (world < 0 || (world > 0 && world > ctx->gather_world))
    return fail(ctx, POMCP_E_INVALID, "merge_roots: no gather buffer for that many ranks");
  if ((int64_t)(world > 0 ? world : 1) * group > INT32_MAX / 2)
    return fail(ctx, POMCP_E_INVALID, "merge_roots: too many replicas");
  PB_TRY(ctx, hipSetDevice(ctx->device));
  const int G = ctx->dp.B / group;
  const double* src = world > 0 ? ctx->gather : ctx->dp.merge;
  hipLaunchKernelGGL(k_merge_roots, dim3((unsigned)G), dim3(kWave), 0, ctx->stream, src,
                     (int)ctx->dp.B, (int)ctx->dp.A, (int)ctx->dp.sel, (int)group,
                     world > 0 ? (int)world : 1, ctx->merged);
  PB_TRY(ctx, hipGetLastError());
  if (!out) return POMCP_OK;
  const int rc = ctx->fetch(out, ctx->merged, (size_t)G);
  if (rc != POMCP_OK) return rc;
  return first_error(ctx, G, [&](int g) { return out[g].error; }, [](int g, int e) {
    return "search: planner " + std::to_string(g) + ": replica error " + std::to_string(e);
  });
}

int pomcp_synthetic_obs(pomcp_ctx* ctx, uint64_t env_seed_base, uint64_t* obs_keys_out) {
  if (!ctx) return POMCP_E_INVALID;
  PB_TRY(ctx, hipSetDevice(ctx->device));
  with_env(ctx, [&](auto e) {
    hipLaunchKernelGGL(k_synthetic_obs<decltype(e)>, dim3(grid_blocks(ctx->dp.B)), dim3(256), 0,
                       ctx->stream, ctx->dp, env_seed_base);
  });
  PB_TRY(ctx, hipGetLastError());
  return obs_keys_out ? ctx->fetch(obs_keys_out, ctx->dp.out_obs, (size_t)ctx->dp.B) : POMCP_OK;
}

int pomcp_synthetic_step(pomcp_ctx* ctx, uint64_t env_seed_base, const int32_t* actions,
                         uint64_t* obs_keys_out) {
  if (!ctx || !actions) return POMCP_E_INVALID;
  PB_TRY(ctx, hipSetDevice(ctx->device));
  const int B = ctx->dp.B;
  const int rc = ctx->upload(ctx->dp.in_actions, actions, (size_t)B);
  if (rc != POMCP_OK) return rc;
  with_env(ctx, [&](auto e) {
    hipLaunchKernelGGL(k_synthetic_step<decltype(e)>, dim3(grid_blocks(B)), dim3(256), 0, ctx->stream,
                       ctx->dp, env_seed_base);
  });
  PB_TRY(ctx, hipGetLastError());
  if (obs_keys_out) return ctx->fetch(obs_keys_out, ctx->dp.out_obs, (size_t)B);
  PB_TRY(ctx, hipStreamSynchronize(ctx->stream));   // (`actions` is the caller's memory)
  return POMCP_OK;
}

int pomcp_snapshot(pomcp_ctx* ctx) {
  if (!ctx) return POMCP_E_INVALID;
  PB_TRY(ctx, hipSetDevice(ctx->device));
  const int B = ctx->dp.B;
  std::vector<TreeHdr> h((size_t)B);
  int rc = ctx->fetch(h.data(), ctx->dp.hdr, h.size());
  if (rc != POMCP_OK) return rc;
  for (int t = 0; t < B; ++t) {
    // only the post-initial-update state (no blocks, no log, empty overflow map)
    // is restorable by resetting the header and bumping the map generation
    if (h[t].root_t != 1 || h[t].n_blocks != 0 || h[t].n_log != 0 || h[t].error != 0)
      return fail(ctx, POMCP_E_STATE, "snapshot: every tree must be right after its initial update");
  }
  if (!ctx->snap_hdr) PB_TRY(ctx, hipMalloc(&ctx->snap_hdr, sizeof(TreeHdr) * B));
  if ((rc = ctx->upload(ctx->snap_hdr, h.data(), h.size())) != POMCP_OK) return rc;
  PB_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->have_snapshot = true;
  return POMCP_OK;
}

int pomcp_restore(pomcp_ctx* ctx) {
  if (!ctx) return POMCP_E_INVALID;
  if (!ctx->have_snapshot) return fail(ctx, POMCP_E_STATE, "restore without snapshot");
  PB_TRY(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_restore, dim3(grid_blocks(ctx->dp.B)), dim3(256), 0, ctx->stream, ctx->dp,
                     ctx->snap_hdr);
  PB_TRY(ctx, hipGetLastError());
  ctx->defer_pending = false;   // back to the post-update roots: no records left
  return POMCP_OK;
}

// ------------------------------------------------------------ batched episodes

static unsigned episode_blocks(int B) { return (unsigned)((B + kEpThreads - 1) / kEpThreads); }
// (groups of root-parallel replicas: one wave per group)
static unsigned group_blocks(int G) { return (unsigned)((G + kEpGroupWaves - 1) / kEpGroupWaves); }

int pomcp_episodes_set_group(pomcp_ctx* ctx, int32_t group) {
  if (!ctx) return POMCP_E_INVALID;
  if (group < 1 || ctx->dp.B % group != 0)
    return fail(ctx, POMCP_E_INVALID, "episodes_set_group: group must divide num_trees");
  ctx->ep_group_want = group;   // from the next pomcp_episodes_begin on
  return POMCP_OK;
}

int pomcp_episodes_begin(pomcp_ctx* ctx, const uint64_t* env_seeds, const double* pow_table,
                         int32_t max_steps, int32_t until) {
  if (!ctx) return POMCP_E_INVALID;
  if (!env_seeds || !pow_table || max_steps < 1 ||
      (until != POMCP_UNTIL_AGENT_DONE && until != POMCP_UNTIL_ALL_DONE))
    return fail(ctx, POMCP_E_INVALID, "episodes_begin: bad arguments");
  if (ctx->dp.tm && !ctx->tm_set)
    return fail(ctx, POMCP_E_STATE, "episodes_begin: pomcp_set_type_policies first");
  const int K = ctx->ep_group_want;
  if (K > 1 && (ctx->ep_track || ctx->ep_acc_want))
    return fail(ctx, POMCP_E_UNSUPPORTED,
                "episodes_begin: groups of root-parallel replicas (pomcp_episodes_set_group) play "
                "without pomcp_episodes_track_states and pomcp_episodes_track_belief_acc");
  PB_TRY(ctx, hipSetDevice(ctx->device));
  const int B = ctx->dp.B;
  const int G = B / K;   // episodes: one per group of K replicas (K = 1: per tree)
  EpDev& ep = ctx->ep;
  const size_t nB = (size_t)B;
  // (the counts: a workgroup of k_episode_step, or of k_group_episode_step for
  // the most groups a batch can have, B / 2)
  const unsigned nparts = std::max(episode_blocks(B), group_blocks(B / 2));
  int rc = ctx->prepare(ctx, nB, nparts, ctx->dp.in_actions, ctx->dp.in_obs, max_steps, until);
  if (rc != POMCP_OK) return rc;
  if (!ep.kept && (rc = ctx->alloc(ep.kept, nB)) != POMCP_OK) return rc;
  ep.states = nullptr;
  if (ctx->ep_track) {
    if ((rc = ensure_belief_buffers(ctx)) != POMCP_OK) return rc;
    ep.states = ctx->bel_q;
  }
  ep.acc_part = nullptr;
  ep.acc_nparts = 0;
  ctx->ep_acc = false;
  if (ctx->ep_acc_want) {
    EpAccDev& acc = ctx->acc;
    for (hipEvent_t& e : ctx->acc_ev)
      if (!e) PB_TRY(ctx, hipEventCreate(&e));
    if ((rc = ensure_belief_buffers(ctx)) != POMCP_OK) return rc;
    ep.states = ctx->bel_q;
    const int nparts = B < kBelMaxGrid ? B : kBelMaxGrid;
    constexpr size_t kPi = sizeof(ctx->host_other_pi) / sizeof(double);
    if (!acc.part &&   // (the last one allocated)
        ((rc = ctx->alloc(acc.rec, nB)) != POMCP_OK || (rc = ctx->alloc(acc.other_pi, kPi)) != POMCP_OK ||
         (rc = ctx->alloc(acc.part, (size_t)nparts)) != POMCP_OK))
      return rc;
    const int64_t want = ctx->ep_acc_steps_want ? (int64_t)B * max_steps * 3 : 0;
    if (want > ctx->acc_steps_cap) {
      // (an earlier, smaller table stays allocated until the context goes)
      if ((rc = ctx->alloc(ctx->acc_steps_buf, (size_t)want)) != POMCP_OK) return rc;
      ctx->acc_steps_cap = want;
    }
    acc.steps = ctx->ep_acc_steps_want ? ctx->acc_steps_buf : nullptr;
    acc.st = ep.st;
    acc.ps = ep.ps;
    acc.states = ctx->bel_q;
    // particles carry a policy on a type-based context that draws one per particle
    acc.num_other = ctx->dp.tm && !ctx->host_tm.no_mixture_draw ? ctx->host_tm.n_other : 0;
    acc.max_steps = max_steps;
    if ((rc = ctx->upload(acc.other_pi, &ctx->host_other_pi[0][0], kPi)) != POMCP_OK) return rc;
    PB_TRY(ctx, hipMemsetAsync(acc.rec, 0, sizeof(pomcp_episode_belief_acc) * nB, ctx->stream));
    PB_TRY(ctx, hipMemsetAsync(acc.part, 0, sizeof(int32_t) * (size_t)nparts, ctx->stream));
    ep.acc_part = acc.part;
    ep.acc_nparts = nparts;
  }
  if (K > 1 && !ctx->ep_kept_merged &&
      (rc = ctx->alloc(ctx->ep_kept_merged, (size_t)(B / 2))) != POMCP_OK)
    return rc;
  ctx->ep_active = false;
  if ((rc = pomcp_reset(ctx)) != POMCP_OK) return rc;   // (ends queue mode too)
  if ((rc = ctx->upload_tables(ctx, env_seeds, (size_t)G, pow_table)) != POMCP_OK) return rc;
  PB_TRY(ctx, hipMemsetAsync(ep.kept, 0, sizeof(pomcp_root_stats) * nB, ctx->stream));
  if (K > 1) {
    ctx->gr.merged = ctx->merged;
    ctx->gr.kept = ctx->ep_kept_merged;
    ctx->gr.K = K;
    ctx->gr.G = G;
    ctx->gr.num_sims = 0;
    ctx->gr.pad = 0;
    PB_TRY(ctx, hipMemsetAsync(ctx->ep_kept_merged, 0, sizeof(pomcp_merged_root) * (size_t)G,
                               ctx->stream));
    with_episode_env(ctx, [&](auto e) {
      hipLaunchKernelGGL(k_group_episode_reset<decltype(e)>, dim3(group_blocks(G)),
                         dim3(kEpThreads), 0, ctx->stream, ctx->dp, ep, ctx->gr);
    });
  } else {
    with_episode_env(ctx, [&](auto e) {
      hipLaunchKernelGGL(k_episode_reset<decltype(e)>, dim3(episode_blocks(B)), dim3(kEpThreads), 0,
                         ctx->stream, ctx->dp, ep);
    });
  }
  PB_TRY(ctx, hipGetLastError());
  // the tables were copied from the caller's memory: finish before returning
  PB_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->begun();
  ctx->ep_group = K;
  ctx->ep_acc = ctx->ep_acc_want;
  ctx->ep_acc_ms = 0.0;
  return POMCP_OK;
}

int pomcp_episodes_step(pomcp_ctx* ctx, int32_t num_sims, int32_t* live_out) {
  if (!ctx) return POMCP_E_INVALID;
  if (num_sims < 0 || !live_out) return fail(ctx, POMCP_E_INVALID, "episodes_step: bad arguments");
  if (!ctx->ep_active) return fail(ctx, POMCP_E_STATE, "episodes_step: pomcp_episodes_begin first");
  const int K = ctx->ep_group;   // > 1: groups of root-parallel replicas
  if (K > 1 && (int64_t)K * num_sims > INT32_MAX)
    return fail(ctx, POMCP_E_INVALID, "episodes_step: group * num_sims overflows the statistics");
  PB_TRY(ctx, hipSetDevice(ctx->device));
  const int B = ctx->dp.B;
  const int G = B / K;
  const bool reroot = ctx->ep_steps > 0;   // not the batch's first step
  PB_TRY(ctx, hipEventRecord(ctx->ep_ev[0], ctx->stream));
  int rc = launch_update(ctx, reroot);
  if (rc != POMCP_OK) return rc;
  ctx->defer_pending = false;   // k_compact_log materialised the surviving deferred children
  ctx->have_root = true;
  PB_TRY(ctx, hipEventRecord(ctx->ep_ev[1], ctx->stream));
  if ((rc = launch_search(ctx, num_sims, 1)) != POMCP_OK) return rc;
  if (K > 1) {
    // every group's merged decision, left on the device (pomcp_merge_roots, world = 0)
    hipLaunchKernelGGL(k_merge_roots, dim3((unsigned)G), dim3(kWave), 0, ctx->stream,
                       (const double*)ctx->dp.merge, (int)B, (int)ctx->dp.A, (int)ctx->dp.sel, (int)K,
                       1, ctx->merged);
    PB_TRY(ctx, hipGetLastError());
  }
  PB_TRY(ctx, hipEventRecord(ctx->ep_ev[2], ctx->stream));
  const unsigned nblk = K > 1 ? group_blocks(G) : episode_blocks(B);
  if (K > 1) {
    ctx->gr.num_sims = num_sims;
    with_episode_env(ctx, [&](auto e) {
      hipLaunchKernelGGL(k_group_episode_step<decltype(e)>, dim3(nblk), dim3(kEpThreads), 0,
                         ctx->stream, ctx->dp, ctx->ep, ctx->gr);
    });
  } else {
    with_episode_env(ctx, [&](auto e) {
      hipLaunchKernelGGL(k_episode_step<decltype(e)>, dim3(nblk), dim3(kEpThreads), 0, ctx->stream,
                         ctx->dp, ctx->ep);
    });
  }
  PB_TRY(ctx, hipGetLastError());
  if (ctx->ep_acc) {
    // the accuracies of the trees that played, against what k_episode_step wrote
    PB_TRY(ctx, hipEventRecord(ctx->acc_ev[0], ctx->stream));
    hipLaunchKernelGGL(k_episode_belief_acc, dim3((unsigned)ctx->ep.acc_nparts), dim3(kBelThreads),
                       0, ctx->stream, ctx->dp, ctx->acc);
    PB_TRY(ctx, hipGetLastError());
    PB_TRY(ctx, hipEventRecord(ctx->acc_ev[1], ctx->stream));
  }
  if (ctx->q_active) {
    // the queue: the finished slots ranked, their rows written, the slots
    // refilled or retired, the refilled trees' records out of the shared logs
    // (before the next update's scan and the new episodes' first appends)
    ctx->q.step = ctx->ep_steps;
    PB_TRY(ctx, hipEventRecord(ctx->q_ev[0], ctx->stream));
    // (a queue of groups: the slots are the G groups, then the groups' trees)
    hipLaunchKernelGGL(k_queue_rank, dim3(1), dim3(kRankThreads), 0, ctx->stream, ctx->ep, ctx->q,
                       ctx->gq_active ? G : B);
    PB_TRY(ctx, hipGetLastError());
    if (ctx->gq_active) {
      with_episode_env(ctx, [&](auto e) {
        hipLaunchKernelGGL(k_group_queue_refill<decltype(e)>, dim3(episode_blocks(G)),
                           dim3(kEpThreads), 0, ctx->stream, ctx->dp, ctx->ep, ctx->gr, ctx->q,
                           ctx->gq);
      });
      PB_TRY(ctx, hipGetLastError());
      hipLaunchKernelGGL(k_group_queue_trees, dim3(episode_blocks(B)), dim3(kEpThreads), 0,
                         ctx->stream, ctx->dp, ctx->ep, ctx->q, ctx->gq, (int)K);
    } else {
      with_episode_env(ctx, [&](auto e) {
        hipLaunchKernelGGL(k_queue_refill<decltype(e)>, dim3(nblk), dim3(kEpThreads), 0, ctx->stream,
                           ctx->dp, ctx->ep, ctx->q);
      });
    }
    PB_TRY(ctx, hipGetLastError());
    PB_TRY(ctx, hipEventRecord(ctx->q_ev[1], ctx->stream));
    hipLaunchKernelGGL(k_log_drop, dim3((unsigned)search_waves(B)), dim3(kDropThreads), 0, ctx->stream,
                       ctx->dp, (const uint64_t*)ctx->drop_masks);
    PB_TRY(ctx, hipGetLastError());
    PB_TRY(ctx, hipEventRecord(ctx->q_ev[2], ctx->stream));
  }
  // (the log scan's flag comes back under the step's one synchronise)
  uint32_t lf_fail = 0u;
  if (reroot && !ctx->log_scan_legacy)
    PB_TRY(ctx, hipMemcpyAsync(&lf_fail, ctx->dp.lf_fail, sizeof(uint32_t), hipMemcpyDeviceToHost,
                               ctx->stream));
  int32_t counts[2] = {0, 0};
  if ((rc = ctx->finish_step(ctx, nblk, live_out, counts)) != POMCP_OK) return rc;
  if (ctx->ep_acc &&   // its own figure, not a part of slot 2
      (rc = add_elapsed(ctx, ctx->acc_ev[0], ctx->acc_ev[1], &ctx->ep_acc_ms, &ctx->ep_ms[2])) != POMCP_OK)
    return rc;
  for (int k = 0; ctx->q_active && k < 2; ++k)   // their own figures, not a part of slot 2
    if ((rc = add_elapsed(ctx, ctx->q_ev[k], ctx->q_ev[k + 1], &ctx->q_ms[k], &ctx->ep_ms[2])) != POMCP_OK)
      return rc;
  if (lf_fail != 0u) return fail(ctx, POMCP_E_HIP, "update: the log scan's look-back gave up");
  if (counts[1] != 0) {   // some tree failed: the update's error first, then the search's
    if ((rc = ctx->fetch(ctx->host_upd.data(), ctx->dp.upd_out, 2 * (size_t)B)) != POMCP_OK ||
        (rc = first_update_error(ctx)) != POMCP_OK ||
        (rc = pomcp_get_root_stats(ctx, ctx->host_stats.data())) != POMCP_OK)
      return rc;
    if (ctx->ep_acc) {
      std::vector<pomcp_episode_belief_acc> rec((size_t)B);
      if ((rc = ctx->fetch(rec.data(), ctx->acc.rec, rec.size())) != POMCP_OK) return rc;
      rc = first_error(ctx, B, [&](int t) { return rec[t].error; }, [](int t, int e) {
        return "episodes_step: belief accuracy of tree " + std::to_string(t) + ": error " +
               std::to_string(e) + " (its own, or a particle's policy index out of range)";
      });
      if (rc != POMCP_OK) return rc;
    }
    return fail(ctx, POMCP_E_STATE, "episodes_step: an episode record reports an error");
  }
  return POMCP_OK;
}

int pomcp_episodes_states(pomcp_ctx* ctx, pomcp_episode_state* out) {
  if (!ctx || !out) return POMCP_E_INVALID;
  return ctx->get_states(ctx, "pomcp", out, (size_t)(ctx->dp.B / ctx->ep_group));
}

int pomcp_episodes_results(pomcp_ctx* ctx, pomcp_episode_result* out) {
  if (!ctx || !out) return POMCP_E_INVALID;
  return ctx->get_results(ctx, "pomcp", out, (size_t)(ctx->dp.B / ctx->ep_group));
}

int pomcp_episodes_merged_roots(pomcp_ctx* ctx, pomcp_merged_root* out) {
  if (!ctx || !out) return POMCP_E_INVALID;
  if (!ctx->ep_active || ctx->ep_group < 2)
    return fail(ctx, POMCP_E_STATE, "episodes_merged_roots: pomcp_episodes_set_group(K > 1), then "
                                    "pomcp_episodes_begin");
  PB_TRY(ctx, hipSetDevice(ctx->device));
  return ctx->fetch(out, ctx->ep_kept_merged, (size_t)(ctx->dp.B / ctx->ep_group));
}

int pomcp_episodes_track_states(pomcp_ctx* ctx, int32_t on) {
  if (!ctx || (on != 0 && on != 1)) return POMCP_E_INVALID;
  ctx->ep_track = on != 0;   // from the next pomcp_episodes_begin on
  return POMCP_OK;
}

int pomcp_episodes_belief_stats(pomcp_ctx* ctx, pomcp_belief_counts* out) {
  if (!ctx || !out) return fail(ctx, POMCP_E_INVALID, "episodes_belief_stats: null argument");
  if (!ctx->ep_active || ctx->ep.states == nullptr)
    return fail(ctx, POMCP_E_STATE, "episodes_belief_stats: pomcp_episodes_track_states(1), then "
                                    "pomcp_episodes_begin");
  int rc = belief_stats_ready(ctx);
  if (rc != POMCP_OK) return rc;
  PB_TRY(ctx, hipSetDevice(ctx->device));
  // the query states are on the device already (k_episode_reset / k_episode_step)
  rc = launch_belief_stats(ctx, reinterpret_cast<const uint32_t*>(ctx->bel_q), false);
  if (rc != POMCP_OK) return rc;
  if ((rc = ctx->fetch(out, ctx->bel_out, (size_t)ctx->dp.B)) != POMCP_OK) return rc;
  return first_error(ctx, ctx->dp.B, [&](int t) { return out[t].error; }, [](int t, int e) {
    return "episodes_belief_stats: tree " + std::to_string(t) + ": error " + std::to_string(e);
  });
}

int pomcp_episodes_set_population(pomcp_ctx* ctx, const pomcp_episode_population* pop) {
  if (!ctx) return POMCP_E_INVALID;
  return ctx->set_population(ctx, pop, ctx->dp.A, true);   // from the next pomcp_episodes_begin on
}

int pomcp_episodes_set_population_kinds(pomcp_ctx* ctx, const pomcp_policy_kinds* kinds) {
  if (!ctx) return POMCP_E_INVALID;
  int rc = POMCP_E_INVALID;
  with_episode_env(ctx, [&](auto e) { rc = ctx->template set_population_kinds<decltype(e)>(ctx, kinds); });
  return rc;
}

int pomcp_episodes_pop_states(pomcp_ctx* ctx, pomcp_episode_pop_state* out) {
  if (!ctx || !out) return POMCP_E_INVALID;
  return ctx->get_pop_states(ctx, "pomcp", out, (size_t)(ctx->dp.B / ctx->ep_group));
}

int pomcp_episodes_track_belief_acc(pomcp_ctx* ctx, int32_t on, int32_t per_step) {
  if (!ctx || (on != 0 && on != 1) || (per_step != 0 && per_step != 1)) return POMCP_E_INVALID;
  ctx->ep_acc_want = on != 0;   // from the next pomcp_episodes_begin on
  ctx->ep_acc_steps_want = on != 0 && per_step != 0;
  return POMCP_OK;
}

int pomcp_episodes_belief_acc(pomcp_ctx* ctx, pomcp_episode_belief_acc* out) {
  if (!ctx || !out) return POMCP_E_INVALID;
  if (!ctx->ep_active || !ctx->ep_acc)
    return fail(ctx, POMCP_E_STATE, "episodes_belief_acc: pomcp_episodes_track_belief_acc(1, ..), "
                                    "then pomcp_episodes_begin");
  PB_TRY(ctx, hipSetDevice(ctx->device));
  return ctx->fetch(out, ctx->acc.rec, (size_t)ctx->dp.B);
}

int pomcp_episodes_belief_acc_steps(pomcp_ctx* ctx, double* out) {
  if (!ctx || !out) return POMCP_E_INVALID;
  if (!ctx->ep_active || !ctx->ep_acc || ctx->acc.steps == nullptr)
    return fail(ctx, POMCP_E_STATE, "episodes_belief_acc_steps: pomcp_episodes_track_belief_acc("
                                    "1, 1), then pomcp_episodes_begin");
  PB_TRY(ctx, hipSetDevice(ctx->device));
  return ctx->fetch(out, ctx->acc.steps, 3 * (size_t)ctx->dp.B * (size_t)ctx->acc.max_steps);
}

int pomcp_episodes_belief_acc_ms(pomcp_ctx* ctx, double* ms) {
  if (!ctx || !ms) return POMCP_E_INVALID;
  *ms = ctx->ep_acc_ms;
  return POMCP_OK;
}

int pomcp_episodes_timing(pomcp_ctx* ctx, double ms[3], int32_t* steps) {
  if (!ctx || !ms || !steps) return POMCP_E_INVALID;
  ctx->get_timing(ms, steps);
  return POMCP_OK;
}

// ------------------------------------------------------------ episode queue

static int ensure_drop_masks(pomcp_ctx* ctx) {
  if (ctx->drop_masks) return POMCP_OK;
  return ctx->alloc(ctx->drop_masks, (size_t)search_waves(ctx->dp.B));
}

// Queue mode for the batch pomcp_episodes_begin has just started: `slots` slots
// (the trees, or the groups of a queue of groups) playing entries 0 .. slots - 1
// of the n seeds.  The per-slot arrays are sized for num_trees slots.
static int queue_arm(pomcp_ctx* ctx, const uint64_t* env_seeds, int32_t n, int slots) {
  const int rc = ensure_drop_masks(ctx);
  if (rc != POMCP_OK) return rc;
  ctx->q.drop = ctx->drop_masks;
  ctx->q.acc_in = ctx->ep_acc ? ctx->acc.rec : nullptr;
  ctx->q.acc = ctx->ep_acc ? ctx->acc.rec : nullptr;
  PB_TRY(ctx, hipMemsetAsync(ctx->drop_masks, 0, sizeof(uint64_t) * (size_t)search_waves(ctx->dp.B),
                             ctx->stream));
  return ctx->arm_queue(ctx, env_seeds, n, slots, (size_t)ctx->dp.B);
}

int pomcp_episodes_queue_begin(pomcp_ctx* ctx, const uint64_t* env_seeds, int32_t n,
                               const double* pow_table, int32_t max_steps, int32_t until) {
  if (!ctx) return POMCP_E_INVALID;
  if (!env_seeds || n < ctx->dp.B)
    return fail(ctx, POMCP_E_INVALID, "episodes_queue_begin: the queue needs at least num_trees "
                                      "environment seeds");
  if (ctx->ep_group_want > 1)
    return fail(ctx, POMCP_E_UNSUPPORTED, "episodes_queue_begin: no queue for groups of "
                                          "root-parallel replicas (pomcp_episodes_set_group)");
  const bool steps_want = ctx->ep_acc_steps_want;
  ctx->ep_acc_steps_want = false;   // (no per-step table in queue mode)
  int rc = pomcp_episodes_begin(ctx, env_seeds, pow_table, max_steps, until);
  ctx->ep_acc_steps_want = steps_want;
  if (rc != POMCP_OK) return rc;
  return queue_arm(ctx, env_seeds, n, ctx->dp.B);
}

int pomcp_episodes_group_queue_begin(pomcp_ctx* ctx, int32_t group, const uint64_t* env_seeds,
                                     int32_t n, const double* pow_table, int32_t max_steps,
                                     int32_t until) {
  if (!ctx) return POMCP_E_INVALID;
  if (group < 2 || ctx->dp.B % group != 0)
    return fail(ctx, POMCP_E_INVALID, "episodes_group_queue_begin: group >= 2 must divide "
                                      "num_trees");
  const int G = ctx->dp.B / group;
  if (!env_seeds || n < G)
    return fail(ctx, POMCP_E_INVALID, "episodes_group_queue_begin: the queue needs at least "
                                      "num_trees / group environment seeds");
  if (ctx->ep_track || ctx->ep_acc_want)
    return fail(ctx, POMCP_E_UNSUPPORTED,
                "episodes_group_queue_begin: groups of root-parallel replicas play without "
                "pomcp_episodes_track_states and pomcp_episodes_track_belief_acc");
  int rc;
  if (!ctx->gq.fin_merged &&   // (the last one allocated; the most groups there are)
      ((rc = ctx->alloc(ctx->gq.key, (size_t)(ctx->dp.B / 2))) != POMCP_OK ||
       (rc = ctx->alloc(ctx->gq.fin_merged, (size_t)(ctx->dp.B / 2))) != POMCP_OK))
    return rc;
  // the group size is this call's own: what pomcp_episodes_set_group stored stays
  const int32_t want = ctx->ep_group_want;
  ctx->ep_group_want = group;
  rc = pomcp_episodes_begin(ctx, env_seeds, pow_table, max_steps, until);
  ctx->ep_group_want = want;
  if (rc != POMCP_OK) return rc;
  PB_TRY(ctx, hipMemsetAsync(ctx->gq.fin_merged, 0, sizeof(pomcp_merged_root) * (size_t)G,
                             ctx->stream));
  if ((rc = queue_arm(ctx, env_seeds, n, G)) != POMCP_OK) return rc;
  ctx->gq_active = true;
  return POMCP_OK;
}

// The running queue's slots: the trees, or the groups of a queue of groups.
static size_t queue_slots(const pomcp_ctx* ctx) {
  return (size_t)(ctx->gq_active ? ctx->dp.B / ctx->ep_group : ctx->dp.B);
}

int pomcp_episodes_queue_rows(pomcp_ctx* ctx, pomcp_episode_queue_row* out) {
  if (!ctx || !out) return POMCP_E_INVALID;
  return ctx->get_queue_rows(ctx, "pomcp", out);
}

int pomcp_episodes_queue_slots(pomcp_ctx* ctx, int32_t* out) {
  if (!ctx || !out) return POMCP_E_INVALID;
  return ctx->get_queue_slots(ctx, "pomcp", out, queue_slots(ctx));
}

int pomcp_episodes_queue_finished(pomcp_ctx* ctx, pomcp_episode_state* states_out,
                                  int32_t* queue_index_out) {
  if (!ctx || !states_out || !queue_index_out) return POMCP_E_INVALID;
  return ctx->get_queue_finished(ctx, "pomcp", states_out, queue_index_out, queue_slots(ctx));
}

int pomcp_episodes_queue_finished_merged(pomcp_ctx* ctx, pomcp_merged_root* out) {
  if (!ctx || !out) return POMCP_E_INVALID;
  if (!ctx->ep_active || !ctx->gq_active)
    return fail(ctx, POMCP_E_STATE, "episodes_queue_finished_merged: "
                                    "pomcp_episodes_group_queue_begin first");
  PB_TRY(ctx, hipSetDevice(ctx->device));
  return ctx->fetch(out, (const pomcp_merged_root*)ctx->gq.fin_merged, queue_slots(ctx));
}

int pomcp_episodes_queue_timing(pomcp_ctx* ctx, double ms[2]) {
  if (!ctx || !ms) return POMCP_E_INVALID;
  ctx->get_queue_timing(ms);
  return POMCP_OK;
}

// Debug: one search wave's log, in record order (pomcp_device.h WaveLog).
int pomcp_debug_get_wave_log(pomcp_ctx* ctx, int32_t wave, uint32_t* ids, uint32_t* v0, uint32_t* v1,
                             uint32_t* aux, int32_t capacity, int32_t* count) {
  if (!ctx || !count || wave < 0 || wave >= search_waves(ctx->dp.B) || capacity < 0)
    return POMCP_E_INVALID;
  PB_TRY(ctx, hipSetDevice(ctx->device));
  uint32_t n = 0u;
  int rc = ctx->fetch(&n, (const uint32_t*)ctx->dp.wlog + wave, 1);
  if (rc != POMCP_OK) return rc;
  const int64_t cap = (int64_t)kWave * ctx->dp.Np;
  if ((int64_t)n > cap || n > (uint32_t)INT32_MAX)
    return fail(ctx, POMCP_E_STATE, "get_wave_log: a count beyond the log's capacity");
  *count = (int32_t)n;
  const size_t m = (size_t)((int32_t)n < capacity ? (int32_t)n : capacity);
  if (m == 0) return POMCP_OK;
  if (!ids || !v0 || !v1) return POMCP_E_INVALID;
  if (aux && !ctx->dp.tm) return fail(ctx, POMCP_E_STATE, "get_wave_log: aux needs a type-based context");
  const uint32_t* base = reinterpret_cast<const uint32_t*>(ctx->dp.plog) +
                         (int64_t)wave * (3 + ctx->dp.tm) * cap;
  if ((rc = ctx->fetch(ids, base, m)) != POMCP_OK || (rc = ctx->fetch(v0, base + cap, m)) != POMCP_OK ||
      (rc = ctx->fetch(v1, base + 2 * cap, m)) != POMCP_OK)
    return rc;
  return aux ? ctx->fetch(aux, base + 3 * cap, m) : POMCP_OK;
}

// Debug: k_log_drop with the caller's masks.
int pomcp_debug_log_drop(pomcp_ctx* ctx, const uint64_t* masks) {
  if (!ctx || !masks) return POMCP_E_INVALID;
  PB_TRY(ctx, hipSetDevice(ctx->device));
  int rc = ensure_drop_masks(ctx);
  if (rc != POMCP_OK) return rc;
  const int nsw = search_waves(ctx->dp.B);
  if ((rc = ctx->upload((const uint64_t*)ctx->drop_masks, masks, (size_t)nsw)) != POMCP_OK) return rc;
  hipLaunchKernelGGL(k_log_drop, dim3((unsigned)nsw), dim3(kDropThreads), 0, ctx->stream, ctx->dp,
                     (const uint64_t*)ctx->drop_masks);
  PB_TRY(ctx, hipGetLastError());
  PB_TRY(ctx, hipStreamSynchronize(ctx->stream));   // (`masks` is the caller's memory)
  return POMCP_OK;
}

// Debug: the context's Env::step and Env::obs_key on the device, one case per
// lane (k_env_selftest): the device functions k_search steps its trees with.
int pomcp_debug_env_step(pomcp_ctx* ctx, const uint32_t* in, int32_t n, uint32_t* out) {
  if (!ctx || !in || !out || n <= 0) return POMCP_E_INVALID;
  PB_TRY(ctx, hipSetDevice(ctx->device));
  uint32_t *din = nullptr, *dout = nullptr;
  PB_TRY(ctx, hipMalloc(&din, sizeof(uint32_t) * 5 * (size_t)n));
  hipError_t e = hipMalloc(&dout, sizeof(uint32_t) * 8 * (size_t)n);
  if (e == hipSuccess) e = hipMemcpyAsync(din, in, sizeof(uint32_t) * 5 * (size_t)n, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    with_env(ctx, [&](auto env) {
      hipLaunchKernelGGL(k_env_selftest<decltype(env)>, grid, block, 0, ctx->stream, ctx->dp.model,
                         ctx->dp.ego, (const uint32_t*)din, (int)n, dout);
    });
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, dout, sizeof(uint32_t) * 8 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(din);
  (void)hipFree(dout);
  PB_TRY(ctx, e);
  return POMCP_OK;
}

// Debug: FP64 sqrt / div / add-mul on the device, for bit-exactness checks
// against the host (include/pomcp_debug.h).
int pomcp_debug_fp_selftest(const double* a, const double* b, int32_t n, double* out) {
  if (!a || !b || !out || n <= 0) return POMCP_E_INVALID;
  double *da = nullptr, *db = nullptr, *dout = nullptr;
  if (hipMalloc(&da, sizeof(double) * n) != hipSuccess) return POMCP_E_HIP;
  (void)hipMalloc(&db, sizeof(double) * n);
  (void)hipMalloc(&dout, sizeof(double) * 4 * n);
  (void)hipMemcpy(da, a, sizeof(double) * n, hipMemcpyHostToDevice);
  (void)hipMemcpy(db, b, sizeof(double) * n, hipMemcpyHostToDevice);
  hipLaunchKernelGGL(k_fp_selftest, dim3((n + 255) / 256), dim3(256), 0, 0, da, db, n, dout);
  hipError_t e = hipMemcpy(out, dout, sizeof(double) * 4 * n, hipMemcpyDeviceToHost);
  (void)hipFree(da);
  (void)hipFree(db);
  (void)hipFree(dout);
  return e == hipSuccess ? POMCP_OK : POMCP_E_HIP;
}

// Debug: rcp_nr / rsq_nr (the fast UCB scores' 1/x and 1/sqrt(x)) on the
// device, for the error bound their exact fallback relies on.
int pomcp_debug_fast_recip(const double* x, int32_t n, double* out) {
  if (!x || !out || n <= 0) return POMCP_E_INVALID;
  double *dx = nullptr, *dout = nullptr;
  if (hipMalloc(&dx, sizeof(double) * n) != hipSuccess) return POMCP_E_HIP;
  if (hipMalloc(&dout, sizeof(double) * 2 * n) != hipSuccess) {
    (void)hipFree(dx);
    return POMCP_E_HIP;
  }
  (void)hipMemcpy(dx, x, sizeof(double) * n, hipMemcpyHostToDevice);
  hipLaunchKernelGGL(k_fast_recip, dim3((n + 255) / 256), dim3(256), 0, 0, dx, n, dout);
  hipError_t e = hipMemcpy(out, dout, sizeof(double) * 2 * n, hipMemcpyDeviceToHost);
  (void)hipFree(dx);
  (void)hipFree(dout);
  return e == hipSuccess ? POMCP_OK : POMCP_E_HIP;
}

// Debug: device exp (the I-NTMCP softmax, intmcp.py:784-786) for comparison
// with the host's math.exp.
int pomcp_debug_exp(const double* x, int32_t n, double* out) {
  if (!x || !out || n <= 0) return POMCP_E_INVALID;
  double *dx = nullptr, *dout = nullptr;
  if (hipMalloc(&dx, sizeof(double) * n) != hipSuccess) return POMCP_E_HIP;
  (void)hipMalloc(&dout, sizeof(double) * n);
  (void)hipMemcpy(dx, x, sizeof(double) * n, hipMemcpyHostToDevice);
  hipLaunchKernelGGL(k_exp_selftest, dim3((n + 255) / 256), dim3(256), 0, 0, dx, n, dout);
  hipError_t e = hipMemcpy(out, dout, sizeof(double) * n, hipMemcpyDeviceToHost);
  (void)hipFree(dx);
  (void)hipFree(dout);
  return e == hipSuccess ? POMCP_OK : POMCP_E_HIP;
}


// Debug: k_search's fast-selection margin (pomcp_debug.h); >= 1e-12 keeps
// results exact, larger sends more selections to the exact FP64 scores
// (counted in pomcp_root_stats.n_exact_selects).
// Device time of k_belief_stats alone: `reps` launches between two events on the
// context stream, after one untimed launch (tools/belief_stats_timing.py).
int pomcp_debug_belief_stats_ms(pomcp_ctx* ctx, const uint32_t* states, int32_t reps,
                                float* ms_per_launch) {
  if (!ctx || !ms_per_launch || reps < 1) return POMCP_E_INVALID;
  int rc = belief_stats_ready(ctx);
  if (rc != POMCP_OK) return rc;
  PB_TRY(ctx, hipSetDevice(ctx->device));
  rc = launch_belief_stats(ctx, states);
  if (rc != POMCP_OK) return rc;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  PB_TRY(ctx, hipEventCreate(&e0));
  hipError_t e = hipEventCreate(&e1);
  if (e == hipSuccess) e = hipEventRecord(e0, ctx->stream);
  for (int32_t r = 0; r < reps && e == hipSuccess; ++r) {
    rc = launch_belief_stats(ctx, states, false);
    if (rc != POMCP_OK) break;
  }
  if (e == hipSuccess && rc == POMCP_OK) e = hipEventRecord(e1, ctx->stream);
  if (e == hipSuccess && rc == POMCP_OK) e = hipEventSynchronize(e1);
  float ms = 0.f;
  if (e == hipSuccess && rc == POMCP_OK) e = hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (rc != POMCP_OK) return rc;
  if (e != hipSuccess) return fail(ctx, POMCP_E_HIP, std::string("belief_stats_ms: ") + hipGetErrorString(e));
  *ms_per_launch = ms / (float)reps;
  return POMCP_OK;
}

int pomcp_debug_set_select_margin(pomcp_ctx* ctx, double rel) {
  if (!ctx || !(rel >= 1e-12) || !(rel <= 1.0)) return POMCP_E_INVALID;
  ctx->dp.sel_margin = rel;
  return POMCP_OK;
}

// Debug: use only the first n (1..6) inline obs slots of every action node, so
// the overflow map serves the rest (tests of that path: the models here rarely
// give an action node more than 6 obs children).  Before the first search.
int pomcp_debug_set_inline_slots(pomcp_ctx* ctx, int32_t n) {
  if (!ctx || n < 1 || n > kSlots) return POMCP_E_INVALID;
  ctx->dp.islots = n;
  return POMCP_OK;
}

// Debug: every tree's overflow-map generation (TreeHdr.epoch) becomes gen[b]
// (1..kEpochMask); the maps themselves are not touched, so entries already
// stored under gen[b] would read as live again.  Tests of the generation wrap.
int pomcp_debug_set_map_generation(pomcp_ctx* ctx, const int32_t* gen) {
  if (!ctx || !gen) return POMCP_E_INVALID;
  const int B = ctx->dp.B;
  for (int t = 0; t < B; ++t)
    if (gen[t] < 1 || gen[t] > (int32_t)kEpochMask)
      return fail(ctx, POMCP_E_INVALID, "debug_set_map_generation: tree " + std::to_string(t) +
                                            ": a generation outside 1.." + std::to_string(kEpochMask));
  PB_TRY(ctx, hipSetDevice(ctx->device));
  std::vector<TreeHdr> h((size_t)B);
  int rc = ctx->fetch(h.data(), ctx->dp.hdr, h.size());   // (synchronises the stream)
  if (rc != POMCP_OK) return rc;
  for (int t = 0; t < B; ++t) h[(size_t)t].epoch = gen[t];
  if ((rc = ctx->upload(ctx->dp.hdr, h.data(), h.size())) != POMCP_OK) return rc;
  PB_TRY(ctx, hipStreamSynchronize(ctx->stream));   // (`h` is local memory)
  return POMCP_OK;
}

// Debug: one tree's overflow map counted on the host: out = {slots of the
// tree's current generation, slots of any other non-zero generation, the
// current generation}.
int pomcp_debug_map_scan(pomcp_ctx* ctx, int32_t tree, int64_t out[3]) {
  if (!ctx || !out || tree < 0 || tree >= ctx->dp.B) return POMCP_E_INVALID;
  TreeHdr h;
  int rc = fetch_hdr(ctx, tree, &h);
  if (rc != POMCP_OK) return rc;
  std::vector<OvfSlot> map((size_t)ctx->dp.H);
  if ((rc = ctx->fetch(map.data(), ctx->dp.ovf + (int64_t)tree * ctx->dp.H, map.size())) != POMCP_OK)
    return rc;
  int64_t live = 0, stale = 0;
  for (const OvfSlot& s : map) {
    const uint32_t g = (uint32_t)(s.key >> kEpochShift);
    if (g == (uint32_t)h.epoch) ++live;
    else if (g != 0u) ++stale;
  }
  out[0] = live;
  out[1] = stale;
  out[2] = h.epoch;
  return POMCP_OK;
}

// Debug: k_search_lds's bound on waiting for a step-tree hand-off (polls; 0 =
// the default), so a test can make every hand-off late.
int pomcp_debug_set_spin_limit(pomcp_ctx* ctx, int32_t polls) {
  if (!ctx || polls < 0) return POMCP_E_INVALID;
  ctx->dp.spin_max = polls;
  return POMCP_OK;
}

// Debug: per-wave phase cycles of k_search (diagnostics build only).
int pomcp_debug_phase_timing(pomcp_ctx* ctx, uint64_t* out, int32_t capacity, int32_t* count) {
  if (!ctx || !count) return POMCP_E_INVALID;
#if !defined(POMCP_PHASE_TIMING) && !defined(PB_CLOG_TIMING)
  (void)out;
  (void)capacity;
  *count = 0;
  return POMCP_E_UNSUPPORTED;
#else
  const int64_t waves = search_waves(ctx->dp.B);
  if (ctx->dp.timing == nullptr) {   // first call: allocate; the next search fills it
    if (ctx->alloc(ctx->dp.timing, 16 * (size_t)waves) != POMCP_OK) return POMCP_E_HIP;
    PB_TRY(ctx, hipMemset(ctx->dp.timing, 0, sizeof(uint64_t) * 16 * (size_t)waves));
    *count = 0;
    return POMCP_OK;
  }
  *count = (int32_t)(16 * waves);
  if (out && capacity >= *count) {
    PB_TRY(ctx, hipStreamSynchronize(ctx->stream));
    PB_TRY(ctx, hipMemcpy(out, ctx->dp.timing, sizeof(uint64_t) * 16 * (size_t)waves,
                          hipMemcpyDeviceToHost));
  }
  return POMCP_OK;
#endif
}

}  // extern "C"

// I-NTMCP (include/intmcp.h)
#include "intmcp_capi.hip"
