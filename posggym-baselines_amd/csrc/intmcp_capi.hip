// C-ABI host side of the I-NTMCP engine (include/intmcp.h).  Part of the
// single translation unit of pomcp_capi.hip.
#include "../../include/intmcp.h"
#include "host_ctx.h"
#include "host_episodes.h"

struct intmcp_ctx : HostCtx, EpisodeHost {
  intmcp_config cfg;
  ImParams ip{};
  std::vector<int32_t> host_out;
  std::vector<IHdr> host_hdr;
  intmcp_root_stats* dev_rstats = nullptr;   // device staging of intmcp_get_root_stats
  // batched episodes (intmcp_episodes_begin / _step; EpisodeHost holds the batch
  // -- EpDev as the POMCP layer's, without root statistics, query states or
  // belief accuracy -- the population and the queue): the pairs' side records
  // and whether the batch has ended (its parked pairs restored)
  intmcp_episode_kept* ep_kept = nullptr;   // [B]
  bool ep_ended = false;
  // the per-pair reset (intmcp_reset_pairs, the episode queue): the pairs to
  // reset and their count, on the device
  int32_t* rp_list = nullptr;   // [B]
  int32_t* rp_cnt = nullptr;    // [1]
  // the episode queue's (q_ms = {rank + list + refill, the arena clear}, q_ev[0 .. 3])
  int64_t* q_cleared = nullptr;   // [B] 16 B words the clear stored for each slot's refills
  unsigned long long* dbg_scan = nullptr;   // [3] intmcp_debug_arena_scan's counts
};

// intmcp_root_stats of every pair's planner root (the level-1 root; at nesting
// level 0 the root of tree 1) (was a host loop with two synchronous copies per
// pair: seconds at 65,536 pairs)
__global__ __launch_bounds__(64) void k_im_root_stats(ImParams d, intmcp_root_stats* out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= d.B) return;
  const IHdr h = d.hdr[t];
  const int T = d.nest0 ? 1 : 0;
  const char* const blk = d.nodes + im_node_off(d.Nn, d.B, t, T, h.cur, d.nt);
  const INode node = *reinterpret_cast<const INode*>(blk);
  intmcp_root_stats o;
  memset(&o, 0, sizeof(o));
  o.action = h.last_action;
  o.num_sims = h.num_sims;
  o.search_depth = h.search_depth;
  o.root_visits = node.visits;
  o.root_absorbing = im_absorbing(node.info) ? 1 : 0;
  o.belief_size = h.root_size;
  o.error = h.err;
  const int nr = im_nreg(node.info);
  o.num_children = nr;
  if (im_has_stats(node.info)) {
    const char* rv = blk + im_rec_delta(d.B, t);                   // its action records
    for (int i = 0; i < nr && i < POMCP_MAX_ACTIONS; ++i) {
      const int a = im_order(node.info, i);
      o.child_action[i] = a;
      if (a < d.A) {
        const uint32_t* hv = reinterpret_cast<const uint32_t*>(blk + kImHeads + 12 * a);   // node line
        const uint2 tot = *reinterpret_cast<const uint2*>(rv + kImRec * a);
        o.child_visits[i] = (int)hv[0];
        o.child_values[i] = hilo_d(hv[1], hv[2]);
        o.child_totals[i] = hilo_d(tot.x, tot.y);
      }
    }
  }
  o.min_value = h.mm_min[T];
  o.max_value = h.mm_max[T];
  for (int k = 0; k < 2; ++k) {   // (the first two trees; intmcp_get_tree_counts has them all)
    o.n_nodes[k] = h.n_nodes[k];
    o.n_log[k] = h.n_log[k];
    o.n_stats[k] = h.n_stats[k];
  }
  o.n_support = h.n_sup;
  out[t] = o;
}

static unsigned im_blocks(int B) { return (unsigned)((B + 63) / 64); }

// f(Env{}) with the context's environment (envs.h)
template <class F>
static void im_with_env(const intmcp_ctx* ctx, F&& f) {
  env_dispatch<EnvDriving, EnvPursuitEvasion>(ctx->cfg.base.env_id, f);
}

// The first pair whose status code(t) is an error.
template <class Code>
static int im_first_error(intmcp_ctx* ctx, const char* what, Code code) {
  return first_error(ctx, ctx->ip.B, code, [&](int t, int e) {
    return std::string(what) + ": pair " + std::to_string(t) + ": status " + std::to_string(e);
  });
}

// nodes 0..n-1 of one tree of one pair, packed as [n][kImBlock] (line, then
// the action records; the device layout interleaves them by wave:
// im_node_off, im_rec_delta)
static int im_copy_blocks(intmcp_ctx* ctx, std::vector<char>& out, int pair, int tree, int n) {
  out.resize((size_t)n * kImBlock);
  if (n == 0) return POMCP_OK;
  const char* line0 = ctx->ip.nodes + im_node_off(ctx->ip.Nn, ctx->ip.B, pair, tree, 0, ctx->ip.nt);
  const size_t ns = (size_t)im_node_stride(ctx->ip.B, pair);
  PB_TRY(ctx, hipMemcpy2DAsync(out.data(), kImBlock, line0, ns, kImLine, n, hipMemcpyDeviceToHost,
                               ctx->stream));
  PB_TRY(ctx, hipMemcpy2DAsync(out.data() + kImLine, kImBlock, line0 + im_rec_delta(ctx->ip.B, pair),
                               ns, kImRecs, n, hipMemcpyDeviceToHost, ctx->stream));
  PB_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return POMCP_OK;
}

// batched episodes: a pair per lane of 256-lane workgroups (intmcp_episode.hip)
static unsigned im_episode_blocks(int B) { return (unsigned)((B + kEpThreads - 1) / kEpThreads); }

// f(Env{}) with the context's environment as the episode kernels know it (episode_step.h)
template <class F>
static void im_with_episode_env(const intmcp_ctx* ctx, F&& f) {
  env_dispatch<EpDriving, EpPursuitEvasion>(ctx->cfg.base.env_id, f);
}

extern "C" {

// ctx == NULL: why the last intmcp_create of this thread failed
static thread_local std::string g_create_err;
const char* intmcp_last_error(const intmcp_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

void intmcp_destroy(intmcp_ctx* ctx) {
  if (!ctx) return;
  ctx->close();
  ctx->destroy_events();
  delete ctx;
}

int intmcp_create(const intmcp_config* cfg, int32_t device, void* hip_stream, intmcp_ctx** out) {
  if (!cfg || !out) return POMCP_E_INVALID;
  *out = nullptr;
  const pomcp_config& c = cfg->base;
  g_create_err.clear();
  auto bad = [&](int code, const char* m) {
    g_create_err = m;
    return code;
  };
  if (c.abi_version != POMCP_ABI_VERSION) return bad(POMCP_E_INVALID, "ABI version mismatch");
  if (c.env_id != POMCP_ENV_DRIVING && c.env_id != POMCP_ENV_PURSUIT_EVASION)
    return bad(POMCP_E_UNSUPPORTED, "env_id");   // (CooperativeReaching-v0 included: lane POMCP only)
  if (c.num_agents != 2) return bad(POMCP_E_UNSUPPORTED, "2 agents");
  if (c.num_actions != (c.env_id == POMCP_ENV_DRIVING ? 5 : 4)) return bad(POMCP_E_INVALID, "num_actions");
  if (c.action_selection != POMCP_SEL_UCB && c.action_selection != POMCP_SEL_UNIFORM)
    return bad(POMCP_E_UNSUPPORTED, "I-NTMCP pucb reads self.action_space (intmcp.py:645): ucb / uniform only");
  if (c.ego_agent < 0 || c.ego_agent > 1 || c.num_trees < 1) return bad(POMCP_E_INVALID, "ego / pairs");
  if (cfg->nesting_level < 0 || cfg->nesting_level > kImMaxT - 1)
    return bad(POMCP_E_UNSUPPORTED, "nesting levels 0 to INTMCP_MAX_TREES - 1 (5)");
  if (c.depth_limit < 0 || c.step_limit < 0 || c.num_particles < 1) return bad(POMCP_E_INVALID, "limits");
  if (cfg->max_nodes < 2 || cfg->max_nodes >= (1ll << 28) || cfg->max_stats < c.num_actions ||
      cfg->max_log < 1 || cfg->hash_slots < 16 || (cfg->hash_slots & (cfg->hash_slots - 1)) ||
      cfg->hash_slots > (1ll << 31) || cfg->max_root_belief < 2 * (c.num_particles + c.extra_particles) ||
      cfg->max_support_particles < 1)
    return bad(POMCP_E_INVALID, "capacities");
  if (!c.log_table || c.log_table_size < 2 || !c.discount_pow || c.discount_pow_size < 1)
    return bad(POMCP_E_INVALID, "tables");
  auto* ctx = new intmcp_ctx();
  ctx->cfg = *cfg;
  int rc = ctx->open(device, hip_stream);
  if (rc != POMCP_OK) {
    delete ctx;
    return rc;
  }
  ctx->set_env_model(c);
  ImParams& d = ctx->ip;
  d.fast_slack = IM_FAST_SLACK;
  d.B = c.num_trees;
  d.A = c.num_actions;
  // nesting level 0: the planner's tree is tree 1, whose agent is p.other
  d.nest0 = cfg->nesting_level == 0 ? 1 : 0;
  d.nt = cfg->nesting_level >= 2 ? cfg->nesting_level + 1 : 2;   // a tree per level (nesting 0: 2)
  d.ego = d.nest0 ? 1 - c.ego_agent : c.ego_agent;
  d.other = 1 - d.ego;
  d.sel = c.action_selection;
  d.depth_limit = c.depth_limit;
  d.step_limit = c.step_limit;
  d.n_target = c.num_particles + c.extra_particles;
  d.extra = c.extra_particles;
  d.has_kb = c.has_known_bounds;
  d.state_belief_only = cfg->state_belief_only;
  d.discount = c.discount;
  d.c = c.c;
  d.limit_factor = c.reinvigoration_sample_limit_factor;
  d.kb_min = c.known_min;
  d.kb_max = c.known_max;
  d.Nn = cfg->max_nodes;
  d.Ns = cfg->max_stats;
  d.Nl = cfg->max_log;
  d.H = cfg->hash_slots;
  d.Nr = cfg->max_root_belief;
  d.Nsp = cfg->max_support_particles;
  const int64_t B = c.num_trees;
  // (the first failure skips the rest)
  auto alloc = [&](auto*& field, int64_t count) {
    if (rc == POMCP_OK) rc = ctx->alloc(field, (size_t)count);
  };
  alloc(d.hdr, B);
  d.nstride = kImBlock;   // node blocks (intmcp.hip), interleaved by wave: im_node_off
  alloc(d.nodes, B * d.nt * d.Nn * d.nstride);
  alloc(d.hash, B * d.nt * d.H);
  alloc(d.log, B * d.nt * d.Nl);
  alloc(d.root, B * 2 * d.Nr);
  alloc(d.sup, B * 2 * d.Nr);
  alloc(d.supp, B * 2 * d.Nsp);
  for (int m = 0; m < kImMaxMid; ++m) {   // the middle planners' beliefs and distributions
    const bool mid = m < d.nt - 2;
    alloc(d.msup[m], mid ? B * 2 * d.Nr : 1);
    alloc(d.msupp[m], mid ? B * 2 * d.Nsp : 1);
    alloc(d.mprob[m], mid ? B * d.Nr : 1);
  }
  alloc(d.path, B * kImPath * 3);
  alloc(d.prob, B * d.Nr);
  alloc(d.logtab, c.log_table_size);
  alloc(d.dpow, c.discount_pow_size);
  if (rc == POMCP_OK) rc = ctx->alloc_bytes(d.model, ctx->model_bytes);
  alloc(d.in_actions, B);
  alloc(d.in_obs, B);
  alloc(d.out, B * 2);
  alloc(d.out_obs, B);
  if (rc != POMCP_OK) {
    g_create_err = ctx->err;
    intmcp_destroy(ctx);
    return rc;
  }
  d.logtab_n = c.log_table_size;
  d.dpow_n = (int32_t)(c.discount_pow_size > INT32_MAX ? INT32_MAX : c.discount_pow_size);
  std::vector<IHdr> h((size_t)B);
  for (int64_t t = 0; t < B; ++t) {
    std::memset(&h[t], 0, sizeof(IHdr));
    h[t].seed = c.seed;
    h[t].tree_key = c.tree_key_base + (uint32_t)t;
  }
  if (ctx->upload(d.logtab, c.log_table, (size_t)c.log_table_size) != POMCP_OK ||
      ctx->upload(d.dpow, c.discount_pow, (size_t)c.discount_pow_size) != POMCP_OK ||
      ctx->upload_bytes(d.model, ctx->host_model, ctx->model_bytes) != POMCP_OK ||
      ctx->upload(d.hdr, h.data(), (size_t)B) != POMCP_OK ||
      hipStreamSynchronize(ctx->stream) != hipSuccess) {
    g_create_err = "initial upload failed";
    intmcp_destroy(ctx);
    return POMCP_E_HIP;
  }
  ctx->host_out.resize((size_t)(2 * B));
  ctx->host_hdr.resize((size_t)B);
  rc = intmcp_reset(ctx);
  if (rc != POMCP_OK) {
    g_create_err = "reset: " + ctx->err;
    intmcp_destroy(ctx);
    return rc;
  }
  *out = ctx;
  return POMCP_OK;
}

int intmcp_reset(intmcp_ctx* ctx) {
  if (!ctx) return POMCP_E_INVALID;
  PB_TRY(ctx, hipSetDevice(ctx->device));
  ctx->ep_active = false;   // a batch of episodes ends with its trees
  ctx->q_active = false;    // and its queue
  // node lines and records start zeroed: statistics and inline child slots
  // need no initialising writes (intmcp.hip, kImBlock)
  PB_TRY(ctx, hipMemsetAsync(ctx->ip.nodes, 0, (size_t)ctx->ip.B * ctx->ip.nt * ctx->ip.Nn * kImBlock,
                             ctx->stream));
  const int64_t slots = (int64_t)ctx->ip.B * ctx->ip.nt * ctx->ip.H;
  const int64_t cblocks = std::min<int64_t>((slots + 255) / 256, 256 * 64);
  hipLaunchKernelGGL(k_im_clear_hash, dim3((unsigned)cblocks), dim3(256), 0, ctx->stream, ctx->ip.hash,
                     slots);
  im_with_env(ctx, [&](auto e) {
    hipLaunchKernelGGL(k_im_reset<decltype(e)>, dim3(im_blocks(ctx->ip.B)), dim3(64), 0, ctx->stream,
                       ctx->ip);
  });
  PB_TRY(ctx, hipGetLastError());
  PB_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return POMCP_OK;
}

// INTMCP.update's kernel for every pair, on the inputs in ip.in_actions /
// ip.in_obs (intmcp_update uploads them; a batched episode step leaves them
// there).
static int im_launch_update(intmcp_ctx* ctx) {
  const int B = ctx->ip.B;
  // a wave per pair for few pairs (the drop-in): the update's log scans are
  // shared by the wave's lanes (k_im_update kWave); a lane per pair otherwise
  const bool wave = B <= 1024;
  const dim3 ugrid(wave ? (unsigned)B : (unsigned)im_blocks(B));
  im_with_env(ctx, [&](auto e) {
    dispatch<std::false_type, std::true_type>(wave, [&](auto w) {
      using E = decltype(e);
      constexpr bool W = decltype(w)::value;
      if (ctx->ip.nt == 2)   // nesting levels 0 and 1
        hipLaunchKernelGGL((k_im_update<E, W>), ugrid, dim3(64), 0, ctx->stream, ctx->ip);
      else   // a tree per nesting level from level 2
        dispatch<Int<3>, Int<4>, Int<5>, Int<6>>(ctx->ip.nt - 3, [&](auto nt) {
          hipLaunchKernelGGL((k_im_updateN<E, decltype(nt)::value, W>), ugrid, dim3(64), 0, ctx->stream,
                             ctx->ip);
        });
    });
  });
  PB_TRY(ctx, hipGetLastError());
  return POMCP_OK;
}

int intmcp_update(intmcp_ctx* ctx, const int32_t* actions, const uint64_t* obs_keys,
                  int32_t* root_absorbing_out) {
  if (!ctx || !obs_keys) return POMCP_E_INVALID;
  PB_TRY(ctx, hipSetDevice(ctx->device));
  const int B = ctx->ip.B;
  std::vector<int32_t> acts((size_t)B, -1);
  if (actions) std::memcpy(acts.data(), actions, sizeof(int32_t) * (size_t)B);
  int rc;
  if ((rc = ctx->upload(ctx->ip.in_actions, acts.data(), (size_t)B)) != POMCP_OK ||
      (rc = ctx->upload(ctx->ip.in_obs, obs_keys, (size_t)B)) != POMCP_OK)
    return rc;
  if ((rc = im_launch_update(ctx)) != POMCP_OK) return rc;
  if ((rc = ctx->fetch(ctx->host_out.data(), ctx->ip.out, 2 * (size_t)B)) != POMCP_OK) return rc;
  if (root_absorbing_out)
    for (int t = 0; t < B; ++t) root_absorbing_out[t] = ctx->host_out[2 * t];
  return im_first_error(ctx, "update", [&](int t) { return ctx->host_out[2 * (size_t)t + 1]; });
}

static int im_fetch_hdr(intmcp_ctx* ctx) {
  return ctx->fetch(ctx->host_hdr.data(), ctx->ip.hdr, (size_t)ctx->ip.B);
}

// The actions of a finished search from the pairs' headers, or its first error.
static int im_search_actions(intmcp_ctx* ctx, int32_t* actions_out) {
  int rc = im_fetch_hdr(ctx);
  if (rc != POMCP_OK) return rc;
  rc = im_first_error(ctx, "search", [&](int t) { return ctx->host_hdr[t].err; });
  if (rc != POMCP_OK) return rc;
  for (int t = 0; t < ctx->ip.B; ++t) actions_out[t] = ctx->host_hdr[t].last_action;
  return POMCP_OK;
}

// one launch of sims[l] simulations at level l (l = 0 .. nt - 1 in turn; nt >= 3)
static int im_searchN(intmcp_ctx* ctx, const int32_t sims[kImMaxT], int32_t flags, int32_t* actions_out);

int intmcp_search_levels(intmcp_ctx* ctx, int32_t level0_sims, int32_t level1_sims,
                         int32_t flags, int32_t* actions_out) {
  if (!ctx || level0_sims < 0 || level1_sims < 0 || (flags & ~(kImBegin | kImFinal)))
    return POMCP_E_INVALID;
  if (ctx->ip.nest0 && level1_sims > 0)
    return fail(ctx, POMCP_E_INVALID, "search_levels: nesting level 0 has no level-1 simulations");
  if (ctx->ip.nt >= 3) {
    int32_t sims[kImMaxT] = {};
    sims[0] = level0_sims;
    sims[1] = level1_sims;
    return im_searchN(ctx, sims, flags, actions_out);
  }
  PB_TRY(ctx, hipSetDevice(ctx->device));
  im_with_env(ctx, [&](auto e) {
    hipLaunchKernelGGL(k_im_search<decltype(e)>, dim3(im_blocks(ctx->ip.B)), dim3(64), 0, ctx->stream,
                       ctx->ip, (int)level0_sims, (int)level1_sims, (int)flags);
  });
  PB_TRY(ctx, hipGetLastError());
  return actions_out ? im_search_actions(ctx, actions_out) : POMCP_OK;
}

static int im_searchN(intmcp_ctx* ctx, const int32_t sims[kImMaxT], int32_t flags, int32_t* actions_out) {
  PB_TRY(ctx, hipSetDevice(ctx->device));
  const dim3 grid(im_blocks(ctx->ip.B));
  ImSims s{};
  for (int l = 0; l < ctx->ip.nt; ++l) s.s[l] = sims[l];
  im_with_env(ctx, [&](auto e) {   // a tree per nesting level
    dispatch<Int<3>, Int<4>, Int<5>, Int<6>>(ctx->ip.nt - 3, [&](auto nt) {
      hipLaunchKernelGGL((k_im_searchN<decltype(e), decltype(nt)::value>), grid, dim3(64), 0, ctx->stream,
                         ctx->ip, s, (int)flags);
    });
  });
  PB_TRY(ctx, hipGetLastError());
  return actions_out ? im_search_actions(ctx, actions_out) : POMCP_OK;
}

// intmcp_search's launch alone: num_sims simulations at every level, BEGIN | FINAL
static int im_launch_search(intmcp_ctx* ctx, int32_t num_sims) {
  return intmcp_search(ctx, num_sims, nullptr);
}

int intmcp_search(intmcp_ctx* ctx, int32_t num_sims, int32_t* actions_out) {
  if (!ctx || num_sims < 0) return POMCP_E_INVALID;
  if (ctx->ip.nt >= 3) {
    int32_t sims[kImMaxT] = {};
    for (int l = 0; l < ctx->ip.nt; ++l) sims[l] = num_sims;
    return im_searchN(ctx, sims, kImBegin | kImFinal, actions_out);
  }
  return intmcp_search_levels(ctx, num_sims, ctx->ip.nest0 ? 0 : num_sims, kImBegin | kImFinal,
                              actions_out);
}

int intmcp_search_level(intmcp_ctx* ctx, int32_t level, int32_t sims, int32_t flags,
                        int32_t* actions_out) {
  if (!ctx || sims < 0 || (flags & ~(kImBegin | kImFinal))) return POMCP_E_INVALID;
  const int top = ctx->ip.nest0 ? 0 : ctx->ip.nt - 1;   // the planner's nesting level
  if (level < 0 || level > top)
    return fail(ctx, POMCP_E_INVALID, "search_level: no level " + std::to_string(level));
  if (ctx->ip.nt >= 3) {
    int32_t s[kImMaxT] = {};
    s[level] = sims;
    return im_searchN(ctx, s, flags, actions_out);
  }
  return intmcp_search_levels(ctx, level == 0 ? sims : 0, level == 1 ? sims : 0, flags, actions_out);
}

int intmcp_get_root_stats(intmcp_ctx* ctx, intmcp_root_stats* out) {
  if (!ctx || !out) return POMCP_E_INVALID;
  PB_TRY(ctx, hipSetDevice(ctx->device));
  const int B = ctx->ip.B;
  int rc;
  if (!ctx->dev_rstats && (rc = ctx->alloc(ctx->dev_rstats, (size_t)B)) != POMCP_OK) return rc;
  // one lane per pair gathers its root's record, then a single copy
  hipLaunchKernelGGL(k_im_root_stats, dim3(im_blocks(B)), dim3(64), 0, ctx->stream, ctx->ip,
                     ctx->dev_rstats);
  PB_TRY(ctx, hipGetLastError());
  if ((rc = ctx->fetch(out, ctx->dev_rstats, (size_t)B)) != POMCP_OK) return rc;
  // a failed search (arena, depleted root, ...) is reported here, as
  // pomcp_get_root_stats does: its partial tree's action must not be used
  return im_first_error(ctx, "search", [&](int t) { return out[t].error; });
}

int intmcp_get_root_belief(intmcp_ctx* ctx, int32_t pair, uint32_t* out, int32_t capacity,
                           int32_t* count) {
  if (!ctx || !count || pair < 0 || pair >= ctx->ip.B) return POMCP_E_INVALID;
  int rc = im_fetch_hdr(ctx);
  if (rc != POMCP_OK) return rc;
  const IHdr& h = ctx->host_hdr[pair];
  *count = h.root_size;
  if (!out || capacity < h.root_size) return POMCP_OK;
  std::vector<uint4> buf((size_t)h.root_size);
  rc = ctx->fetch(buf.data(), ctx->ip.root + ((int64_t)pair * 2 + h.root_sel) * ctx->ip.Nr,
               (size_t)h.root_size);
  if (rc != POMCP_OK) return rc;
  for (int i = 0; i < h.root_size; ++i) {
    out[3 * i] = buf[i].x;
    out[3 * i + 1] = buf[i].y;
    out[3 * i + 2] = buf[i].z;
  }
  return POMCP_OK;
}

int intmcp_get_nodes(intmcp_ctx* ctx, int32_t pair, int32_t tree, void* out, int32_t capacity,
                     int32_t* count) {
  if (!ctx || !count || pair < 0 || pair >= ctx->ip.B || tree < 0 || tree >= ctx->ip.nt)
    return POMCP_E_INVALID;
  int rc = im_fetch_hdr(ctx);
  if (rc != POMCP_OK) return rc;
  const int n = ctx->host_hdr[pair].n_nodes[tree];
  *count = n;
  if (!out || capacity < n) return POMCP_OK;
  // the 32 B record of include/intmcp.h from each node's INode and ICold
  // (layout: intmcp.hip ImPair::N, ImPair::C)
  const int64_t ns = kImBlock;
  std::vector<char> blocks;
  rc = im_copy_blocks(ctx, blocks, pair, tree, n);
  if (rc != POMCP_OK) return rc;
  struct NodeRec {
    int32_t parent;
    uint32_t info;
    int32_t visits, t, stats;
    uint32_t support;
    uint64_t okey;
  };
  NodeRec* o = reinterpret_cast<NodeRec*>(out);
  for (int i = 0; i < n; ++i) {
    INode x;
    ICold c;
    std::memcpy(&x, blocks.data() + (size_t)i * ns, sizeof(INode));
    std::memcpy(&c, blocks.data() + (size_t)i * ns + kImCold, sizeof(ICold));
    o[i] = NodeRec{x.parent, x.info & ~kImStatsBit, x.visits, x.t, c.stats, c.support, c.okey};
  }
  return POMCP_OK;
}

int intmcp_get_stats(intmcp_ctx* ctx, int32_t pair, int32_t tree, void* out, int32_t capacity,
                     int32_t* count) {
  if (!ctx || !count || pair < 0 || pair >= ctx->ip.B || tree < 0 || tree >= ctx->ip.nt)
    return POMCP_E_INVALID;
  int rc = im_fetch_hdr(ctx);
  if (rc != POMCP_OK) return rc;
  const int n = ctx->host_hdr[pair].n_stats[tree];
  *count = n;
  if (!out || capacity < n) return POMCP_OK;
  // statistics in allocation order (INode.stats = their first index), gathered
  // from the node blocks
  const int nn = ctx->host_hdr[pair].n_nodes[tree];
  const int64_t ns = kImBlock;
  std::vector<char> blocks;
  rc = im_copy_blocks(ctx, blocks, pair, tree, nn);
  if (rc != POMCP_OK) return rc;
  IStat* o = reinterpret_cast<IStat*>(out);
  for (int i = 0; i < nn; ++i) {
    const char* bk = blocks.data() + (size_t)i * ns;   // head {visits, value}; record {total, ...}
    ICold c;
    std::memcpy(&c, bk + kImCold, sizeof(ICold));
    if (c.stats < 0) continue;
    for (int a = 0; a < ctx->ip.A && c.stats + a < n; ++a) {
      IStat st;
      std::memcpy(&st.visits, bk + kImHeads + 12 * (size_t)a, 4);
      st.pad = 0;
      std::memcpy(&st.value, bk + kImHeads + 12 * (size_t)a + 4, 8);
      std::memcpy(&st.total, bk + kImLine + kImRec * (size_t)a, 8);
      st.agg = 0.0;   // not kept
      o[c.stats + a] = st;
    }
  }
  return POMCP_OK;
}

// Debug: per-pair phase cycles of k_im_search (diagnostics build only): the
// first call allocates and zeroes the counters; later searches add to them.
int intmcp_debug_phase_timing(intmcp_ctx* ctx, uint64_t* out, int32_t capacity, int32_t* count) {
  if (!ctx || !count) return POMCP_E_INVALID;
#ifndef POMCP_PHASE_TIMING
  (void)out;
  (void)capacity;
  *count = 0;
  return POMCP_E_UNSUPPORTED;
#else
  const size_t n = (size_t)kImPhases * (size_t)ctx->ip.B;
  if (ctx->ip.timing == nullptr) {
    if (ctx->alloc(ctx->ip.timing, n) != POMCP_OK) return POMCP_E_HIP;
    PB_TRY(ctx, hipMemset(ctx->ip.timing, 0, sizeof(uint64_t) * n));
    *count = 0;
    return POMCP_OK;
  }
  *count = (int32_t)n;
  if (out && capacity >= *count) {
    PB_TRY(ctx, hipStreamSynchronize(ctx->stream));
    PB_TRY(ctx, hipMemcpy(out, ctx->ip.timing, sizeof(uint64_t) * n, hipMemcpyDeviceToHost));
  }
  return POMCP_OK;
#endif
}

// Debug: the other agent's softmax fast path (ImPair::sample_action) with its
// bound widened `slack` times (>= 1 keeps results exact; a large slack sends
// most draws to the exact FP64 path); from this call on, exact-path draws are
// counted (intmcp_debug_exact_draws).
int intmcp_debug_set_softmax_slack(intmcp_ctx* ctx, float slack) {
  if (!ctx || !(slack >= 1.0f)) return POMCP_E_INVALID;
  if (ctx->ip.exact_draws == nullptr) {
    if (ctx->alloc(ctx->ip.exact_draws, 1) != POMCP_OK) return POMCP_E_HIP;
    PB_TRY(ctx, hipMemsetAsync(ctx->ip.exact_draws, 0, sizeof(unsigned long long), ctx->stream));
  }
  ctx->ip.fast_slack = slack;
  return POMCP_OK;
}

int intmcp_set_search_policy(intmcp_ctx* ctx, int32_t level, int32_t agent, const double* probs) {
  if (!ctx || agent < 0 || agent > 1) return POMCP_E_INVALID;
  const int top = ctx->ip.nest0 ? 0 : ctx->ip.nt - 1;   // the planner's nesting level
  if (level < 0 || level > top)
    return fail(ctx, POMCP_E_INVALID, "set_search_policy: no planner at level " + std::to_string(level));
  const int k = top - level;               // tree 0 = the top level; the level-0 planner's is the last
  const int tree = ctx->ip.nest0 ? 1 : k;
  ImParams& d = ctx->ip;
  if (probs == nullptr) {
    d.sp_fixed[tree][agent] = 0;
  } else {
    // random.choices' cumulative weights, summed left to right as
    // itertools.accumulate does, and total = cum[-1] + 0.0
    double acc = 0.0;
    for (int a = 0; a < d.A; ++a) {
      if (!(probs[a] >= 0.0))
        return fail(ctx, POMCP_E_INVALID, "set_search_policy: negative or NaN weight");
      acc = a == 0 ? probs[0] : acc + probs[a];
      d.sp_cum[tree][agent][a] = acc;
    }
    if (!(acc > 0.0)) return fail(ctx, POMCP_E_INVALID, "set_search_policy: weights sum to zero");
    d.sp_tot[tree][agent] = acc + 0.0;
    d.sp_fixed[tree][agent] = 1;
  }
  d.sp_any = 0;
  for (int t = 0; t < kImMaxT; ++t)
    for (int i = 0; i < 2; ++i) d.sp_any |= d.sp_fixed[t][i];
  return POMCP_OK;
}

int intmcp_debug_exact_draws(intmcp_ctx* ctx, uint64_t* count) {
  if (!ctx || !count) return POMCP_E_INVALID;
  *count = 0;
  if (ctx->ip.exact_draws == nullptr) return POMCP_OK;
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "exact-draw counter");
  return ctx->fetch(reinterpret_cast<unsigned long long*>(count), ctx->ip.exact_draws, 1);
}

int intmcp_get_support(intmcp_ctx* ctx, int32_t pair, int32_t* entries, int32_t capacity_entries,
                       int32_t* n_entries, uint32_t* particles, int32_t capacity_particles,
                       int32_t* n_particles) {
  if (!ctx || !n_entries || !n_particles || pair < 0 || pair >= ctx->ip.B) return POMCP_E_INVALID;
  int rc = im_fetch_hdr(ctx);
  if (rc != POMCP_OK) return rc;
  const IHdr& h = ctx->host_hdr[pair];
  *n_entries = h.n_sup;
  *n_particles = h.sup_used;
  if (entries && capacity_entries >= h.n_sup) {
    rc = ctx->fetch(reinterpret_cast<ISup*>(entries),
                 ctx->ip.sup + ((int64_t)pair * 2 + h.sup_sel) * ctx->ip.Nr, (size_t)h.n_sup);
    if (rc != POMCP_OK) return rc;
  }
  if (particles && capacity_particles >= h.sup_used) {
    rc = ctx->fetch(reinterpret_cast<uint2*>(particles),
                 ctx->ip.supp + ((int64_t)pair * 2 + h.sup_sel) * ctx->ip.Nsp, (size_t)h.sup_used);
    if (rc != POMCP_OK) return rc;
  }
  return POMCP_OK;
}

int intmcp_get_middle_support(intmcp_ctx* ctx, int32_t pair, int32_t tree, int32_t* entries,
                              int32_t capacity_entries, int32_t* n_entries, uint32_t* particles,
                              int32_t capacity_particles, int32_t* n_particles) {
  if (!ctx || !n_entries || !n_particles || pair < 0 || pair >= ctx->ip.B) return POMCP_E_INVALID;
  if (tree < 1 || tree > ctx->ip.nt - 2)
    return fail(ctx, POMCP_E_INVALID,
                "get_middle_support: no middle tree " + std::to_string(tree) + " (nesting levels >= 2)");
  int rc = im_fetch_hdr(ctx);
  if (rc != POMCP_OK) return rc;
  const IHdr& h = ctx->host_hdr[pair];
  const int m = tree - 1;
  *n_entries = h.n_msup[m];
  *n_particles = h.msup_used[m];
  if (entries && capacity_entries >= h.n_msup[m]) {
    rc = ctx->fetch(reinterpret_cast<ISup*>(entries),
                 ctx->ip.msup[m] + ((int64_t)pair * 2 + h.msel[m]) * ctx->ip.Nr, (size_t)h.n_msup[m]);
    if (rc != POMCP_OK) return rc;
  }
  if (particles && capacity_particles >= h.msup_used[m]) {
    std::vector<uint4> buf((size_t)h.msup_used[m]);
    rc = ctx->fetch(buf.data(), ctx->ip.msupp[m] + ((int64_t)pair * 2 + h.msel[m]) * ctx->ip.Nsp,
                 (size_t)h.msup_used[m]);
    if (rc != POMCP_OK) return rc;
    for (int i = 0; i < h.msup_used[m]; ++i) {
      particles[3 * i] = buf[i].x;
      particles[3 * i + 1] = buf[i].y;
      particles[3 * i + 2] = buf[i].z;
    }
  }
  return POMCP_OK;
}

int intmcp_get_mid_support(intmcp_ctx* ctx, int32_t pair, int32_t* entries, int32_t capacity_entries,
                           int32_t* n_entries, uint32_t* particles, int32_t capacity_particles,
                           int32_t* n_particles) {
  return intmcp_get_middle_support(ctx, pair, 1, entries, capacity_entries, n_entries, particles,
                                   capacity_particles, n_particles);
}

int intmcp_get_tree_counts(intmcp_ctx* ctx, int32_t* out) {
  if (!ctx || !out) return POMCP_E_INVALID;
  int rc = im_fetch_hdr(ctx);
  if (rc != POMCP_OK) return rc;
  for (int t = 0; t < ctx->ip.B; ++t) {
    const IHdr& h = ctx->host_hdr[t];
    for (int k = 0; k < kImMaxT; ++k) {
      const bool on = k < ctx->ip.nt;
      out[3 * kImMaxT * t + 3 * k] = on ? h.n_nodes[k] : 0;
      out[3 * kImMaxT * t + 3 * k + 1] = on ? h.n_log[k] : 0;
      out[3 * kImMaxT * t + 3 * k + 2] = on ? h.n_stats[k] : 0;
    }
  }
  return POMCP_OK;
}

int intmcp_synthetic_obs(intmcp_ctx* ctx, uint64_t env_seed_base, uint64_t* obs_keys_out) {
  if (!ctx) return POMCP_E_INVALID;
  PB_TRY(ctx, hipSetDevice(ctx->device));
  im_with_env(ctx, [&](auto e) {
    hipLaunchKernelGGL(k_im_synthetic<decltype(e)>, dim3(im_blocks(ctx->ip.B)), dim3(64), 0, ctx->stream,
                       ctx->ip, env_seed_base);
  });
  PB_TRY(ctx, hipGetLastError());
  if (obs_keys_out) return ctx->fetch(obs_keys_out, ctx->ip.out_obs, (size_t)ctx->ip.B);
  PB_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return POMCP_OK;
}

// ------------------------------------------------------------ batched episodes

int intmcp_episodes_set_population(intmcp_ctx* ctx, const pomcp_episode_population* pop) {
  if (!ctx) return POMCP_E_INVALID;
  return ctx->set_population(ctx, pop, ctx->ip.A, false);   // from the next intmcp_episodes_begin on
}

int intmcp_episodes_begin(intmcp_ctx* ctx, const uint64_t* env_seeds, const double* pow_table,
                          int32_t max_steps, int32_t until) {
  if (!ctx) return POMCP_E_INVALID;
  if (!env_seeds || !pow_table || max_steps < 1 ||
      (until != POMCP_UNTIL_AGENT_DONE && until != POMCP_UNTIL_ALL_DONE))
    return fail(ctx, POMCP_E_INVALID, "episodes_begin: bad arguments");
  PB_TRY(ctx, hipSetDevice(ctx->device));
  const int B = ctx->ip.B;
  const size_t nB = (size_t)B;
  EpDev& ep = ctx->ep;
  int rc = ctx->prepare(ctx, nB, im_episode_blocks(B), ctx->ip.in_actions, ctx->ip.in_obs, max_steps,
                        until);
  if (rc != POMCP_OK) return rc;
  if (!ctx->ep_kept && (rc = ctx->alloc(ctx->ep_kept, nB)) != POMCP_OK) return rc;
  if ((rc = intmcp_reset(ctx)) != POMCP_OK) return rc;   // (ends an earlier batch)
  if ((rc = ctx->upload_tables(ctx, env_seeds, nB, pow_table)) != POMCP_OK) return rc;
  im_with_episode_env(ctx, [&](auto e) {
    hipLaunchKernelGGL(k_im_episode_reset<decltype(e)>, dim3(im_episode_blocks(B)), dim3(kEpThreads),
                       0, ctx->stream, ctx->ip, ep, ctx->ep_kept);
  });
  PB_TRY(ctx, hipGetLastError());
  // the tables were copied from the caller's memory: finish before returning
  PB_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->begun();
  ctx->ep_ended = false;
  return POMCP_OK;
}

int intmcp_episodes_step(intmcp_ctx* ctx, int32_t num_sims, int32_t* live_out) {
  if (!ctx) return POMCP_E_INVALID;
  if (num_sims < 0 || !live_out) return fail(ctx, POMCP_E_INVALID, "episodes_step: bad arguments");
  if (!ctx->ep_active) return fail(ctx, POMCP_E_STATE, "episodes_step: intmcp_episodes_begin first");
  if (ctx->ep_ended)
    return fail(ctx, POMCP_E_STATE, "episodes_step: intmcp_episodes_results ended the batch");
  PB_TRY(ctx, hipSetDevice(ctx->device));
  const int B = ctx->ip.B;
  int rc;
  PB_TRY(ctx, hipEventRecord(ctx->ep_ev[0], ctx->stream));
  if ((rc = im_launch_update(ctx)) != POMCP_OK) return rc;
  PB_TRY(ctx, hipEventRecord(ctx->ep_ev[1], ctx->stream));
  if ((rc = im_launch_search(ctx, num_sims)) != POMCP_OK) return rc;
  PB_TRY(ctx, hipEventRecord(ctx->ep_ev[2], ctx->stream));
  const unsigned nblk = im_episode_blocks(B);
  im_with_episode_env(ctx, [&](auto e) {
    hipLaunchKernelGGL(k_im_episode_step<decltype(e)>, dim3(nblk), dim3(kEpThreads), 0, ctx->stream,
                       ctx->ip, ctx->ep, ctx->ep_kept);
  });
  PB_TRY(ctx, hipGetLastError());
  if (ctx->q_active) {
    // the queue: the finished slots ranked, the refilled ones listed, their
    // arenas cleared (while the headers still hold the old episodes' node
    // counts), then their rows written, their headers reset and their new
    // episodes started
    ctx->q.step = ctx->ep_steps;
    PB_TRY(ctx, hipEventRecord(ctx->q_ev[0], ctx->stream));
    hipLaunchKernelGGL(k_queue_rank, dim3(1), dim3(kRankThreads), 0, ctx->stream, ctx->ep, ctx->q, B);
    PB_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_im_queue_list, dim3(nblk), dim3(kEpThreads), 0, ctx->stream, ctx->q,
                       ctx->rp_list, B);
    PB_TRY(ctx, hipGetLastError());
    PB_TRY(ctx, hipEventRecord(ctx->q_ev[1], ctx->stream));
    hipLaunchKernelGGL(k_im_clear_pairs, dim3(kImClearGrid), dim3(kImClearThreads), 0, ctx->stream,
                       ctx->ip, (const int32_t*)ctx->rp_list, (const int32_t*)(ctx->q.state + 1));
    PB_TRY(ctx, hipGetLastError());
    PB_TRY(ctx, hipEventRecord(ctx->q_ev[2], ctx->stream));
    im_with_episode_env(ctx, [&](auto e) {
      hipLaunchKernelGGL(k_im_queue_refill<decltype(e)>, dim3(nblk), dim3(kEpThreads), 0, ctx->stream,
                         ctx->ip, ctx->ep, ctx->q, ctx->ep_kept, ctx->q_cleared);
    });
    PB_TRY(ctx, hipGetLastError());
    PB_TRY(ctx, hipEventRecord(ctx->q_ev[3], ctx->stream));
  }
  int32_t counts[2] = {0, 0};
  if ((rc = ctx->finish_step(ctx, nblk, live_out, counts)) != POMCP_OK) return rc;
  for (int k = 0; ctx->q_active && k < 3; ++k)   // their own figures, not a part of slot 2
    if ((rc = add_elapsed(ctx, ctx->q_ev[k], ctx->q_ev[k + 1], &ctx->q_ms[k == 1 ? 1 : 0],
                          &ctx->ep_ms[2])) != POMCP_OK)
      return rc;
  if (counts[1] != 0) {   // some pair failed: the update's error first, then the search's
    if ((rc = ctx->fetch(ctx->host_out.data(), ctx->ip.out, 2 * (size_t)B)) != POMCP_OK ||
        (rc = im_first_error(ctx, "update",
                             [&](int t) { return ctx->host_out[2 * (size_t)t + 1]; })) != POMCP_OK ||
        (rc = im_fetch_hdr(ctx)) != POMCP_OK ||
        (rc = im_first_error(ctx, "search", [&](int t) { return ctx->host_hdr[t].err; })) != POMCP_OK)
      return rc;
    return fail(ctx, POMCP_E_STATE, "episodes_step: an episode record reports an error");
  }
  return POMCP_OK;
}

int intmcp_episodes_states(intmcp_ctx* ctx, pomcp_episode_state* out) {
  if (!ctx || !out) return POMCP_E_INVALID;
  return ctx->get_states(ctx, "intmcp", out, (size_t)ctx->ip.B);
}

int intmcp_episodes_results(intmcp_ctx* ctx, pomcp_episode_result* out) {
  if (!ctx || !out) return POMCP_E_INVALID;
  if (!ctx->ep_active) return fail(ctx, POMCP_E_STATE, "episodes_results: intmcp_episodes_begin first");
  PB_TRY(ctx, hipSetDevice(ctx->device));
  // the batch ends: the parked pairs' roots and header fields as their last
  // real steps left them (a later call finds no pair parked)
  hipLaunchKernelGGL(k_im_episode_unpark, dim3(im_episode_blocks(ctx->ip.B)), dim3(kEpThreads), 0,
                     ctx->stream, ctx->ip, ctx->ep_kept);
  PB_TRY(ctx, hipGetLastError());
  ctx->ep_ended = true;
  return ctx->get_results(ctx, "intmcp", out, (size_t)ctx->ip.B);
}

int intmcp_episodes_pop_states(intmcp_ctx* ctx, pomcp_episode_pop_state* out) {
  if (!ctx || !out) return POMCP_E_INVALID;
  return ctx->get_pop_states(ctx, "intmcp", out, (size_t)ctx->ip.B);
}

int intmcp_episodes_timing(intmcp_ctx* ctx, double ms[3], int32_t* steps) {
  if (!ctx || !ms || !steps) return POMCP_E_INVALID;
  ctx->get_timing(ms, steps);
  return POMCP_OK;
}

// ------------------------------------------- per-pair reset, the episode queue

// the device list of the pairs to reset and its count
static int im_ensure_reset_list(intmcp_ctx* ctx) {
  if (ctx->rp_cnt) return POMCP_OK;   // (the last one allocated)
  int rc = ctx->alloc(ctx->rp_list, (size_t)ctx->ip.B);
  return rc != POMCP_OK ? rc : ctx->alloc(ctx->rp_cnt, 1);
}

int intmcp_reset_pairs(intmcp_ctx* ctx, const int32_t* pairs, int32_t n) {
  if (!ctx) return POMCP_E_INVALID;
  const int B = ctx->ip.B;
  if (n < 0 || n > B || (n > 0 && !pairs))
    return fail(ctx, POMCP_E_INVALID, "reset_pairs: 0 to num_pairs indices");
  std::vector<char> seen((size_t)B, 0);
  for (int32_t i = 0; i < n; ++i) {
    if (pairs[i] < 0 || pairs[i] >= B || seen[(size_t)pairs[i]])
      return fail(ctx, POMCP_E_INVALID, "reset_pairs: index " + std::to_string(pairs[i]) +
                                        (pairs[i] < 0 || pairs[i] >= B ? " out of range" : " twice"));
    seen[(size_t)pairs[i]] = 1;
  }
  if (ctx->ep_active && !ctx->ep_ended)
    return fail(ctx, POMCP_E_STATE, "reset_pairs: a batch of episodes is active");
  if (n == 0) return POMCP_OK;
  PB_TRY(ctx, hipSetDevice(ctx->device));
  int rc;
  if ((rc = im_ensure_reset_list(ctx)) != POMCP_OK ||
      (rc = ctx->upload((const int32_t*)ctx->rp_list, pairs, (size_t)n)) != POMCP_OK ||
      (rc = ctx->upload((const int32_t*)ctx->rp_cnt, &n, 1)) != POMCP_OK)
    return rc;
  // the clear reads the node counts the header reset overwrites: in this order
  hipLaunchKernelGGL(k_im_clear_pairs, dim3(kImClearGrid), dim3(kImClearThreads), 0, ctx->stream,
                     ctx->ip, (const int32_t*)ctx->rp_list, (const int32_t*)ctx->rp_cnt);
  PB_TRY(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_im_reset_pairs, dim3(im_blocks(B)), dim3(64), 0, ctx->stream, ctx->ip,
                     (const int32_t*)ctx->rp_list, (const int32_t*)ctx->rp_cnt);
  PB_TRY(ctx, hipGetLastError());
  PB_TRY(ctx, hipStreamSynchronize(ctx->stream));   // (`pairs` and `n` are the caller's memory)
  return POMCP_OK;
}

int intmcp_episodes_queue_begin(intmcp_ctx* ctx, const uint64_t* env_seeds, int32_t n,
                                const double* pow_table, int32_t max_steps, int32_t until) {
  if (!ctx) return POMCP_E_INVALID;
  if (!env_seeds || n < ctx->ip.B)
    return fail(ctx, POMCP_E_INVALID, "episodes_queue_begin: the queue needs at least num_pairs "
                                      "environment seeds");
  int rc = intmcp_episodes_begin(ctx, env_seeds, pow_table, max_steps, until);
  if (rc != POMCP_OK) return rc;
  const size_t nB = (size_t)ctx->ip.B;
  if ((rc = im_ensure_reset_list(ctx)) != POMCP_OK ||
      (!ctx->q_cleared && (rc = ctx->alloc(ctx->q_cleared, nB)) != POMCP_OK))
    return rc;
  ctx->q.drop = nullptr;   // (no shared logs: nothing to drop)
  ctx->q.acc_in = nullptr;
  ctx->q.acc = nullptr;
  PB_TRY(ctx, hipMemsetAsync(ctx->q_cleared, 0, sizeof(int64_t) * nB, ctx->stream));
  return ctx->arm_queue(ctx, env_seeds, n, ctx->ip.B, nB);
}

int intmcp_episodes_queue_rows(intmcp_ctx* ctx, pomcp_episode_queue_row* out) {
  if (!ctx || !out) return POMCP_E_INVALID;
  return ctx->get_queue_rows(ctx, "intmcp", out);
}

int intmcp_episodes_queue_slots(intmcp_ctx* ctx, int32_t* out) {
  if (!ctx || !out) return POMCP_E_INVALID;
  return ctx->get_queue_slots(ctx, "intmcp", out, (size_t)ctx->ip.B);
}

int intmcp_episodes_queue_finished(intmcp_ctx* ctx, pomcp_episode_state* states_out,
                                   int32_t* queue_index_out) {
  if (!ctx || !states_out || !queue_index_out) return POMCP_E_INVALID;
  return ctx->get_queue_finished(ctx, "intmcp", states_out, queue_index_out, (size_t)ctx->ip.B);
}

int intmcp_episodes_queue_timing(intmcp_ctx* ctx, double ms[2]) {
  if (!ctx || !ms) return POMCP_E_INVALID;
  ctx->get_queue_timing(ms);
  return POMCP_OK;
}

// Debug (measurement): the bytes k_im_clear_pairs stored since
// intmcp_episodes_queue_begin, from the per-slot sums k_im_queue_refill keeps.
int intmcp_debug_queue_cleared_bytes(intmcp_ctx* ctx, int64_t* bytes) {
  if (!ctx || !bytes) return POMCP_E_INVALID;
  const int rc0 = ctx->queue_ready(ctx, "intmcp", "debug_queue_cleared_bytes");
  if (rc0 != POMCP_OK) return rc0;
  std::vector<int64_t> words((size_t)ctx->ip.B);
  const int rc = ctx->fetch(words.data(), (const int64_t*)ctx->q_cleared, words.size());
  if (rc != POMCP_OK) return rc;
  int64_t sum = 0;
  for (int64_t w : words) sum += w;
  *bytes = 16 * sum;
  return POMCP_OK;
}

// Debug (tests): what one tree's node arena and obs-child map hold, scanned
// over their whole capacity by one workgroup.
int intmcp_debug_arena_scan(intmcp_ctx* ctx, int32_t pair, int32_t tree, int64_t out[3]) {
  if (!ctx || !out || pair < 0 || pair >= ctx->ip.B || tree < 0 || tree >= ctx->ip.nt)
    return POMCP_E_INVALID;
  PB_TRY(ctx, hipSetDevice(ctx->device));
  int rc;
  if (!ctx->dbg_scan && (rc = ctx->alloc(ctx->dbg_scan, 3)) != POMCP_OK) return rc;
  hipLaunchKernelGGL(k_im_arena_scan, dim3(1), dim3(256), 0, ctx->stream, ctx->ip, (int)pair,
                     (int)tree, ctx->dbg_scan);
  PB_TRY(ctx, hipGetLastError());
  unsigned long long got[3] = {0ull, 0ull, 0ull};
  if ((rc = ctx->fetch(got, (const unsigned long long*)ctx->dbg_scan, 3)) != POMCP_OK) return rc;
  for (int k = 0; k < 3; ++k) out[k] = (int64_t)got[k];
  return POMCP_OK;
}

}  // extern "C"
