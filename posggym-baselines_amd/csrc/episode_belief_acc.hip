// k_episode_belief_acc: BeliefStatTracker.step (utils.py:147-339) for every
// tree of a batch of episodes, accumulated on the device -- the per-episode
// belief_{state,policy,action}_acc columns of run_planning_exp's rows
// (baseline_exps/exp_utils.py:488-534) with nothing per tree on the host
// between steps (pomcp_episodes_track_belief_acc, pomcp.h).
//
// Launched by pomcp_episodes_step after k_episode_step, which has written the
// state the root belief is about (ep.states[b]: the one before the joint
// action), the other agent's action (st[b].last_other_action) and the new
// length (st[b].res.len).  A tree played this step exactly when its record's
// count is below that length; every other tree -- parked, or stopped by an
// error -- is skipped before a particle of it is addressed.
//
// The reduction is k_belief_stats' (bel_count_block, belief_stats.hip): one
// 256-thread workgroup per tree, trees grid-strided, one 16 B record per lane
// and pass, bel_classify per record, __ballot + __popcll into wave-uniform
// integer counts, the four waves' counts joined in LDS.  Thread 0 then does the
// tracker's arithmetic on the totals (bel_accuracy, belief_stats.h: the code
// pomcp_host_belief_acc runs), adds the three values to the tree's sequential
// FP64 sums and stores the record with two 16 B vector stores.  Integers until
// that point, no global atomics, no pre-zeroed output between steps: the same
// bits on every run.  Each workgroup also stores whether any record it owns
// carries an error (acc.part[blockIdx.x]); k_episode_live adds the flags to the
// batch's error count.  Included by pomcp_capi.hip.
#pragma clang fp contract(off)

#include "belief_stats.h"
#include "pomcp_device.h"

namespace pb {

static_assert(sizeof(pomcp_episode_belief_acc) == 32, "belief accuracy record layout");
static_assert(sizeof(pomcp_episode_pop_state) == 8, "population record layout");
static_assert(kBelAccPolicies == kTmMax, "histogram width");

struct EpAccDev {
  pomcp_episode_belief_acc* rec;       // [B]
  double* steps;                       // [B][max_steps][3] {state, policy, action}, or null
  const pomcp_episode_state* st;       // [B] the episode records (k_episode_step's)
  const pomcp_episode_pop_state* ps;   // [B] the true policies' mixture indices
  const uint2* states;                 // [B] the query states (ep.states)
  const double* other_pi;              // [kTmMax][POMCP_MAX_ACTIONS] the planner's, or null
  int32_t* part;                       // [gridDim.x] error flags
  int32_t num_other;                   // policies the particles carry (0: none)
  int32_t max_steps;
};

__global__ __launch_bounds__(kBelThreads) void k_episode_belief_acc(DevParams dp, EpAccDev acc) {
  __shared__ int32_t red[kBelWaves][kBelWords];
  const int lane = lane_id();
  const int wave = uni((int)threadIdx.x / kWave);
  const int num_other = acc.num_other;
  int32_t any_err = 0;
  for (int b = (int)blockIdx.x; b < dp.B; b += (int)gridDim.x) {
    // (every thread reads the record before thread 0 rewrites it: the LDS
    // join's barrier lies between)
    const int4 r1 = reinterpret_cast<const int4*>(acc.rec + b)[1];   // {action_sum, count, error}
    const int count = uni(r1.z);
    const int len = uni(acc.st[b].res.len);
    if (count >= len || count >= acc.max_steps) {   // did not play this step
      any_err |= uni(r1.w) != 0 ? 1 : 0;
      continue;
    }
    const TreeHdr* h = dp.hdr + b;
    int n = uni(h->belief_size);
    const int sel = uni(h->belief_sel);
    int err = uni(h->error);
    if (n < 0 || (int64_t)n > dp.Nr) {   // a header no kernel writes: read nothing
      n = 0;
      if (err == 0) err = POMCP_E_INVALID;
    }
    const uint4* rec = dp.belief + (int64_t)b * dp.Nr + (sel ? dp.Nr - n : 0);
    const uint2 s = acc.states[b];
    const uint32_t q0 = uniu(s.x), q1 = uniu(s.y);
    bel_count_block(rec, n, q0, q1, 1, num_other, lane, wave, red);
    if (threadIdx.x == 0) {
      int32_t tot[kBelWords];
      bel_totals(red, tot);
      if (tot[1] != 0 && err == 0) err = POMCP_E_INVALID;
      double v[3];
      bel_accuracy(n, tot[0], tot + 2, num_other, acc.ps[b].mixture_index,
                   acc.st[b].last_other_action, acc.other_pi, POMCP_MAX_ACTIONS, v);
      const double2 r0 = reinterpret_cast<const double2*>(acc.rec + b)[0];
      double2* o = reinterpret_cast<double2*>(acc.rec + b);
      o[0] = make_double2(r0.x + v[0], r0.y + v[1]);
      const double a_sum = hilo_d((uint32_t)r1.x, (uint32_t)r1.y) + v[2];
      const int e_out = r1.w != 0 ? r1.w : err;
      reinterpret_cast<int4*>(o)[1] =
          make_int4(__double2loint(a_sum), __double2hiint(a_sum), count + 1, e_out);
      if (acc.steps != nullptr) {
        double* p = acc.steps + ((int64_t)b * acc.max_steps + count) * 3;
        p[0] = v[0];
        p[1] = v[1];
        p[2] = v[2];
      }
      any_err |= e_out != 0 ? 1 : 0;
    }
    __syncthreads();   // red is reused by the next tree
  }
  if (threadIdx.x == 0) acc.part[blockIdx.x] = any_err;
}

}  // namespace pb
