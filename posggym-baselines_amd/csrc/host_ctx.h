// The host context the POMCP and I-NTMCP C-ABI layers share (pomcp_capi.hip,
// intmcp_capi.hip): the device and stream of an engine, its device
// allocations, its last error text and the host copy of its environment
// model, with the typed allocate / upload / fetch helpers, the per-tree error
// scan and the compile-time dispatch every entry point is written with.
// Host only; included after host_api.cpp (make_model) in the single
// translation unit.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>
#include <vector>

namespace pb {

// `expr` is a HIP call on behalf of `ctx`: its failure is the context's error
// text and POMCP_E_HIP
#define PB_TRY(ctx, expr)                                                           \
  do {                                                                              \
    hipError_t e_ = (expr);                                                         \
    if (e_ != hipSuccess) {                                                         \
      (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);              \
      return POMCP_E_HIP;                                                           \
    }                                                                               \
  } while (0)

// (hidden: the library exports the C ABI only)
struct __attribute__((visibility("hidden"))) HostCtx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::vector<void*> allocs;
  std::string err;
  DrvModel host_drv;      // the configured environment's device tables
  PeModel host_pe;
  CrModel host_cr;
  PpModel host_pp;
  const void* host_model = nullptr;
  size_t model_bytes = 0;

  // Select the device and take the caller's stream or create one.
  int open(int32_t dev, void* hip_stream) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= dev || dev < 0) return POMCP_E_NO_DEVICE;
    device = dev;
    if (hipSetDevice(dev) != hipSuccess) return POMCP_E_NO_DEVICE;
    if (hip_stream) {
      stream = (hipStream_t)hip_stream;
    } else {
      if (hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) return POMCP_E_HIP;
      own_stream = true;
    }
    return POMCP_OK;
  }

  // Wait for the stream, free every allocation, destroy an owned stream.
  void close() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    for (void* p : allocs) (void)hipFree(p);
    allocs.clear();
    if (own_stream && stream) (void)hipStreamDestroy(stream);
    stream = nullptr;
  }

  // (desc: the description a POMCP_ENV_COOPERATIVE_REACHING (pomcp_cr_grid) or
  // POMCP_ENV_PREDATOR_PREY (pomcp_pp_grid) context is created with,
  // pomcp_create_env; the other environments' travel in the config)
  void set_env_model(const pomcp_config& c, const void* desc = nullptr) {
    if (c.env_id == POMCP_ENV_PREDATOR_PREY) {
      build_pp_model(*static_cast<const pomcp_pp_grid*>(desc), &host_pp);
      host_model = &host_pp;
      model_bytes = sizeof(PpModel);
    } else if (c.env_id == POMCP_ENV_COOPERATIVE_REACHING) {
      build_cr_model(*static_cast<const pomcp_cr_grid*>(desc), &host_cr);
      host_model = &host_cr;
      model_bytes = sizeof(CrModel);
    } else if (c.env_id == POMCP_ENV_PURSUIT_EVASION) {
      build_pe_model(c.pe_grid, &host_pe);
      host_model = &host_pe;
      model_bytes = sizeof(PeModel);
    } else {
      make_model(&c.grid, &host_drv);
      host_model = &host_drv;
      model_bytes = sizeof(DrvModel);
    }
  }

  // Device memory owned by the context (freed by close()); T may be const
  // (the read-only fields of DevParams / ImParams / EpDev) or void.
  template <class T>
  int alloc_bytes(T*& out, size_t bytes) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
    if (e != hipSuccess) {
      err = "hipMalloc(" + std::to_string(bytes) + " B): " + hipGetErrorString(e);
      return POMCP_E_HIP;
    }
    allocs.push_back(p);
    out = static_cast<T*>(p);
    return POMCP_OK;
  }
  template <class T>
  int alloc(T*& out, size_t count) {
    return alloc_bytes(out, sizeof(T) * count);
  }

  // Host to device on the stream; asynchronous: the caller synchronises before
  // `host` goes away.
  int upload_bytes(const void* dev, const void* host, size_t bytes) {
    PB_TRY(this, hipMemcpyAsync(const_cast<void*>(dev), host, bytes, hipMemcpyHostToDevice, stream));
    return POMCP_OK;
  }
  template <class T>
  int upload(const T* dev, const T* host, size_t n) {
    return upload_bytes(dev, host, sizeof(T) * n);
  }

  // Device to host on the stream, complete on return.
  template <class T>
  int fetch(T* host, const T* dev, size_t n) {
    if (n == 0) return POMCP_OK;
    PB_TRY(this, hipMemcpyAsync(host, dev, sizeof(T) * n, hipMemcpyDeviceToHost, stream));
    PB_TRY(this, hipStreamSynchronize(stream));
    return POMCP_OK;
  }
};

// (ctx may be null: the entry points that name their null argument)
static inline int fail(HostCtx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  return code;
}

// The first of n trees / pairs / planners with a non-zero status: code(t) reads
// tree t's, text(t, e) is the context's error; returns that status.
template <class Code, class Text>
static int first_error(HostCtx* ctx, int n, Code code, Text text) {
  for (int t = 0; t < n; ++t) {
    const int e = code(t);
    if (e != 0) return fail(ctx, e, text(t, e));
  }
  return POMCP_OK;
}

// Calls f(Ts{}) for the i-th of Ts: a run-time choice among compile-time
// alternatives (the environment of a kernel template, a tree count, a flag);
// f is a generic lambda, instantiated for every alternative.
template <class... Ts, class F>
static void dispatch(int i, F&& f) {
  int k = 0;
  ((k++ == i ? (void)f(Ts{}) : (void)0), ...);
}
template <int N>
using Int = std::integral_constant<int, N>;
// f(Drv{}) or f(Pe{}) for a pomcp_env: the tags of envs.h or of episode_step.h
template <class Drv, class Pe, class F>
static void env_dispatch(int32_t env, F&& f) {
  dispatch<Drv, Pe>(env == POMCP_ENV_PURSUIT_EVASION ? 1 : 0, f);
}
// the row of a pomcp_env in a table of kernels: Driving, PursuitEvasion,
// CooperativeReaching, PredatorPrey
static inline int env_row(int32_t env) {
  return env == POMCP_ENV_PREDATOR_PREY
             ? 3
             : (env == POMCP_ENV_COOPERATIVE_REACHING ? 2 : (env == POMCP_ENV_PURSUIT_EVASION ? 1 : 0));
}
// the same with f(Cr{}) and f(Pp{}): the layers that run all four environments
template <class Drv, class Pe, class Cr, class Pp, class F>
static void env_dispatch4(int32_t env, F&& f) {
  dispatch<Drv, Pe, Cr, Pp>(env_row(env), f);
}

}  // namespace pb
