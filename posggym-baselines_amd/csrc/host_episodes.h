// The episode host state the POMCP and I-NTMCP C-ABI layers share
// (pomcp_capi.hip, intmcp_capi.hip; a second base of both contexts next to
// HostCtx): the device records of a batch of episodes and of its queue, whether
// they run, the step count and the device time of the phases, the other
// agents' population -- with what both layers do to them around their own
// update / search / step kernels: prepare() before the layer's reset,
// arm_queue() after its begin, finish_step() after its last kernel of a step,
// and the bodies of the getters.  `abi` is the prefix an error text names its
// entry points with ("pomcp" / "intmcp").
// Host only; included after pomcp_episode.hip (EpDev, k_episode_live),
// pomcp_episode_queue.hip (EpQueueDev) and host_ctx.h in the single
// translation unit.
#pragma once

#include "host_ctx.h"

namespace pb {

// *acc += the device milliseconds between two recorded events, which are also
// taken out of *carve (the phase they are a part of), when given
static int add_elapsed(HostCtx* ctx, hipEvent_t from, hipEvent_t to, double* acc,
                       double* carve = nullptr) {
  float ms = 0.f;
  PB_TRY(ctx, hipEventElapsedTime(&ms, from, to));
  *acc += (double)ms;
  if (carve) *carve -= (double)ms;
  return POMCP_OK;
}

struct __attribute__((visibility("hidden"))) EpisodeHost {
  // the batch (<abi>_episodes_begin / _step): the device records, whether a
  // batch is running, its steps so far and the device time of its phases
  // {update, search, the step kernels} between the events [0] .. [3]
  EpDev ep{};
  bool ep_active = false;
  int32_t ep_steps = 0;
  double ep_ms[3] = {0.0, 0.0, 0.0};
  hipEvent_t ep_ev[4] = {nullptr, nullptr, nullptr, nullptr};
  // the other agents' population (<abi>_episodes_set_population): the host's
  // tables and their device copy (every slot's record is ep.ps)
  bool ep_pop_set = false;
  EpPopTables host_pop{};
  EpPopTables* dev_pop = nullptr;
  // the episode queue (<abi>_episodes_queue_begin): whether the running batch
  // has one, its device state and the capacity of its per-entry arrays, the
  // device time of its kernels ({rank + refill, the drop or clear}) and their
  // events (as many as the layer records)
  bool q_active = false;
  EpQueueDev q{};
  int32_t q_cap = 0;
  double q_ms[2] = {0.0, 0.0};
  hipEvent_t q_ev[4] = {nullptr, nullptr, nullptr, nullptr};

  void destroy_events() {
    for (hipEvent_t e : ep_ev)
      if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : q_ev)
      if (e) (void)hipEventDestroy(e);
  }

  // The population of the batches begun from now on (null: the uniform agent);
  // check_mix: the mixture indices must name one of kTmMax policies or none.
  int set_population(HostCtx* ctx, const pomcp_episode_population* pop, int A, bool check_mix) {
    if (!pop) {
      ep_pop_set = false;
      return POMCP_OK;
    }
    EpPopTables t;
    if (!ep_pop_tables(*pop, A, &t))
      return fail(ctx, POMCP_E_INVALID, "episodes_set_population: 1..8 policies, probabilities >= 0 "
                                        "with a positive sum");
    for (int k = 0; check_mix && k < t.n; ++k)
      if (t.mix[k] < -1 || t.mix[k] >= kTmMax)
        return fail(ctx, POMCP_E_INVALID, "episodes_set_population: mixture_index -1..7");
    host_pop = t;
    ep_pop_set = true;
    return POMCP_OK;
  }

  // The kinds of that population's policies (null: all fixed, as set_population
  // leaves them); E: the episode environment of the context.
  template <class E>
  int set_population_kinds(HostCtx* ctx, const pomcp_policy_kinds* kinds) {
    if (!ep_pop_set)
      return fail(ctx, POMCP_E_STATE, "episodes_set_population_kinds: episodes_set_population first");
    EpPopTables t = host_pop;
    const int rc = ep_pop_kinds<E>(kinds, &t);
    if (rc == POMCP_E_UNSUPPORTED)
      return fail(ctx, rc, "episodes_set_population_kinds: the environment has no such reactive "
                           "policy kind (Driving-v1 has the shortest-path agents)");
    if (rc != POMCP_OK)
      return fail(ctx, rc, "episodes_set_population_kinds: kind 0..1, caution 0..15, vmax 0..3");
    host_pop = t;
    return POMCP_OK;
  }

  // What a begin needs before the layer's reset: the events, the records of
  // `slots` trees or pairs (the counts of `nparts` step workgroups), the power
  // table and the population's device copy.  The layer's own records follow.
  int prepare(HostCtx* ctx, size_t slots, size_t nparts, const int32_t* in_actions,
              const uint64_t* in_obs, int32_t max_steps, int32_t until) {
    int rc;
    for (hipEvent_t& e : ep_ev)
      if (!e) PB_TRY(ctx, hipEventCreate(&e));
    if (!ep.out) {   // (the last one allocated: a failed attempt is started over)
      if ((rc = ctx->alloc(ep.st, slots)) != POMCP_OK || (rc = ctx->alloc(ep.ps, slots)) != POMCP_OK ||
          (rc = ctx->alloc(ep.env_seeds, slots)) != POMCP_OK ||
          (rc = ctx->alloc(ep.part, 2 * nparts)) != POMCP_OK)
        return rc;
      ep.in_actions = const_cast<int32_t*>(in_actions);
      ep.in_obs = const_cast<uint64_t*>(in_obs);
      if ((rc = ctx->alloc(ep.out, 2)) != POMCP_OK) return rc;
    }
    // (an earlier, shorter table stays allocated until the context goes)
    if ((ep.pow_table == nullptr || ep.max_steps != max_steps) &&
        (rc = ctx->alloc(ep.pow_table, (size_t)max_steps)) != POMCP_OK)
      return rc;
    ep.max_steps = max_steps;
    ep.until = until;
    ep.pop = nullptr;
    if (ep_pop_set) {
      if ((!dev_pop && (rc = ctx->alloc(dev_pop, 1)) != POMCP_OK) ||
          (rc = ctx->upload(dev_pop, &host_pop, 1)) != POMCP_OK)
        return rc;
      ep.pop = dev_pop;
    }
    return POMCP_OK;
  }

  // After the layer's reset, before its episode reset kernel: the caller's
  // seeds (one per episode) and power table, to the device.
  int upload_tables(HostCtx* ctx, const uint64_t* env_seeds, size_t episodes,
                    const double* pow_table) {
    const int rc = ctx->upload(ep.env_seeds, env_seeds, episodes);
    return rc != POMCP_OK ? rc : ctx->upload(ep.pow_table, pow_table, (size_t)ep.max_steps);
  }

  // The layer's episode reset kernel is done: the batch runs.
  void begun() {
    ep_active = true;
    ep_steps = 0;
    ep_ms[0] = ep_ms[1] = ep_ms[2] = 0.0;
  }

  // Queue mode for the batch just begun: `slots` slots playing entries
  // 0 .. slots - 1 of the n seeds; the per-slot arrays are sized for
  // `slots_alloc`.  The layer has set q.drop / q.acc_in / q.acc and enqueued the
  // clears of its own side arrays: the synchronise here covers them.
  int arm_queue(HostCtx* ctx, const uint64_t* env_seeds, int32_t n, int slots, size_t slots_alloc) {
    int rc;
    for (hipEvent_t& e : q_ev)
      if (!e) PB_TRY(ctx, hipEventCreate(&e));
    if (!q.fin_q) {   // (the last one allocated)
      if ((rc = ctx->alloc(q.slot_q, slots_alloc)) != POMCP_OK ||
          (rc = ctx->alloc(q.slot_ord, slots_alloc)) != POMCP_OK ||
          (rc = ctx->alloc(q.slot_start, slots_alloc)) != POMCP_OK ||
          (rc = ctx->alloc(q.assign, slots_alloc)) != POMCP_OK ||
          (rc = ctx->alloc(q.state, 2)) != POMCP_OK || (rc = ctx->alloc(q.fin, slots_alloc)) != POMCP_OK ||
          (rc = ctx->alloc(q.fin_q, slots_alloc)) != POMCP_OK)
        return rc;
    }
    if (n > q_cap) {   // (an earlier, shorter queue stays allocated until the context goes)
      q_cap = 0;
      if ((rc = ctx->alloc(q.seeds, (size_t)n)) != POMCP_OK ||
          (rc = ctx->alloc(q.rows, (size_t)n)) != POMCP_OK)
        return rc;
      q_cap = n;
    }
    q.n = n;
    q.step = 0;
    std::vector<int32_t> iota((size_t)slots), minus((size_t)slots, -1);
    for (int b = 0; b < slots; ++b) iota[(size_t)b] = b;
    const int32_t state[2] = {slots, 0};
    if ((rc = ctx->upload(q.seeds, env_seeds, (size_t)n)) != POMCP_OK ||
        (rc = ctx->upload((const int32_t*)q.slot_q, iota.data(), (size_t)slots)) != POMCP_OK ||
        (rc = ctx->upload((const int32_t*)q.fin_q, minus.data(), (size_t)slots)) != POMCP_OK ||
        (rc = ctx->upload((const int32_t*)q.state, state, 2)) != POMCP_OK)
      return rc;
    PB_TRY(ctx, hipMemsetAsync(q.slot_ord, 0, sizeof(int32_t) * slots_alloc, ctx->stream));
    PB_TRY(ctx, hipMemsetAsync(q.slot_start, 0, sizeof(int32_t) * slots_alloc, ctx->stream));
    PB_TRY(ctx, hipMemsetAsync(q.rows, 0, sizeof(pomcp_episode_queue_row) * (size_t)n, ctx->stream));
    // (copied from the caller's and local memory: finish before returning)
    PB_TRY(ctx, hipStreamSynchronize(ctx->stream));
    q_ms[0] = q_ms[1] = 0.0;
    q_active = true;
    return POMCP_OK;
  }

  // The end of a step, after the layer's last kernel: the sums of the `nblk`
  // step workgroups' counts, everything copied back under one synchronise (a
  // further word the layer wants under it is enqueued before the call), the
  // step counted, the three phases timed.  counts = {unfinished, errors};
  // *live_out adds the slots the queue refilled (they play on).
  int finish_step(HostCtx* ctx, unsigned nblk, int32_t* live_out, int32_t counts[2]) {
    hipLaunchKernelGGL(k_episode_live, dim3(1), dim3(kEpThreads), 0, ctx->stream, ep, (int)nblk);
    PB_TRY(ctx, hipGetLastError());
    PB_TRY(ctx, hipEventRecord(ep_ev[3], ctx->stream));
    PB_TRY(ctx, hipMemcpyAsync(counts, ep.out, 2 * sizeof(int32_t), hipMemcpyDeviceToHost,
                               ctx->stream));
    int32_t qstate[2] = {0, 0};   // {next, slots refilled this step}
    if (q_active)
      PB_TRY(ctx, hipMemcpyAsync(qstate, q.state, sizeof(qstate), hipMemcpyDeviceToHost,
                                 ctx->stream));
    PB_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ep_steps += 1;
    for (int k = 0; k < 3; ++k) {
      const int rc = add_elapsed(ctx, ep_ev[k], ep_ev[k + 1], &ep_ms[k]);
      if (rc != POMCP_OK) return rc;
    }
    *live_out = counts[0] + qstate[1];
    return POMCP_OK;
  }

  // ---- the getters' bodies (the extern "C" wrappers check their pointers)
  int batch_ready(HostCtx* ctx, const char* abi, const char* what) {
    if (!ep_active)
      return fail(ctx, POMCP_E_STATE, std::string(what) + ": " + abi + "_episodes_begin first");
    PB_TRY(ctx, hipSetDevice(ctx->device));
    return POMCP_OK;
  }
  int queue_ready(HostCtx* ctx, const char* abi, const char* what) {
    if (!ep_active || !q_active)
      return fail(ctx, POMCP_E_STATE, std::string(what) + ": " + abi + "_episodes_queue_begin first");
    PB_TRY(ctx, hipSetDevice(ctx->device));
    return POMCP_OK;
  }
  int get_states(HostCtx* ctx, const char* abi, pomcp_episode_state* out, size_t n) {
    const int rc = batch_ready(ctx, abi, "episodes_states");
    return rc != POMCP_OK ? rc : ctx->fetch(out, (const pomcp_episode_state*)ep.st, n);
  }
  int get_results(HostCtx* ctx, const char* abi, pomcp_episode_result* out, size_t n) {
    std::vector<pomcp_episode_state> st(n);
    const int rc = get_states(ctx, abi, st.data(), n);
    if (rc != POMCP_OK) return rc;
    for (size_t t = 0; t < n; ++t) out[t] = st[t].res;
    return POMCP_OK;
  }
  int get_pop_states(HostCtx* ctx, const char* abi, pomcp_episode_pop_state* out, size_t n) {
    const int rc = batch_ready(ctx, abi, "episodes_pop_states");
    return rc != POMCP_OK ? rc : ctx->fetch(out, (const pomcp_episode_pop_state*)ep.ps, n);
  }
  void get_timing(double ms[3], int32_t* steps) const {
    for (int k = 0; k < 3; ++k) ms[k] = ep_ms[k];
    *steps = ep_steps;
  }
  int get_queue_rows(HostCtx* ctx, const char* abi, pomcp_episode_queue_row* out) {
    const int rc = queue_ready(ctx, abi, "episodes_queue_rows");
    return rc != POMCP_OK ? rc : ctx->fetch(out, (const pomcp_episode_queue_row*)q.rows, (size_t)q.n);
  }
  int get_queue_slots(HostCtx* ctx, const char* abi, int32_t* out, size_t n) {
    const int rc = queue_ready(ctx, abi, "episodes_queue_slots");
    return rc != POMCP_OK ? rc : ctx->fetch(out, (const int32_t*)q.slot_q, n);
  }
  int get_queue_finished(HostCtx* ctx, const char* abi, pomcp_episode_state* states_out,
                     int32_t* queue_index_out, size_t n) {
    int rc = queue_ready(ctx, abi, "episodes_queue_finished");
    if (rc != POMCP_OK ||
        (rc = ctx->fetch(queue_index_out, (const int32_t*)q.fin_q, n)) != POMCP_OK)
      return rc;
    return ctx->fetch(states_out, (const pomcp_episode_state*)q.fin, n);
  }
  void get_queue_timing(double ms[2]) const {
    ms[0] = q_ms[0];
    ms[1] = q_ms[1];
  }
};

}  // namespace pb
