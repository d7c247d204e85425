// bnf_host.h -- what the three units of libbnf_hip.so share on the host: the error text behind bnf_last_error, the small
// launch helpers, and the forecast side's view of a handle.
//
//   bnf_api.hip       the training engine: owns struct bnf_handle, defines fail() and forecast_view()
//   bnf_forecast.hip  the forecast entry points: bnf_handle stays opaque there, a call sees the five fields of Forecast
//   bnf_comm.cpp      the RCCL loader: host only
//
// Nothing in here is exported: the out-of-line functions are hidden, the rest is static inline.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstdio>

#include "../../include/bnf.h"

#define BNF_HIDDEN __attribute__((visibility("hidden")))

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
// formats the calling thread's bnf_last_error text and returns `code` (defined once, in bnf_api.hip)
BNF_HIDDEN int fail(int code, const char* fmt, ...);

#define HIPCHK(expr)                                                                   \
  do {                                                                                 \
    hipError_t _e = (expr);                                                            \
    if (_e != hipSuccess)                                                              \
      return fail(BNF_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                  __FILE__, __LINE__);                                                 \
  } while (0)

static inline int no_device() {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(BNF_ERR_NO_DEVICE, "no HIP device visible: the BayesNF engine has no CPU fallback (needs gfx950)");
  return BNF_OK;
}

// ---------------------------------------------------------------------------
// launch helpers
// ---------------------------------------------------------------------------
static inline unsigned cdiv(int64_t a, int64_t b) { return (unsigned)((a + b - 1) / b); }

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE property of a kernel: remember per
// (kernel instantiation, device) that it has been raised (a process may drive several GPUs).
template <typename K>
static inline void allow_lds(int device, K kernel, int bytes, std::atomic<uint64_t>* done_mask) {
  // (atomic: one host thread per device enqueues through the same launchers -- distributed.run_shards)
  const uint64_t bit = 1ull << (device & 63);
  if (done_mask->load(std::memory_order_relaxed) & bit) return;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e != hipSuccess)
    fprintf(stderr, "[bnf] hipFuncSetAttribute(MaxDynamicSharedMemorySize=%d) failed: %s\n", bytes, hipGetErrorString(e));
  done_mask->fetch_or(bit, std::memory_order_relaxed);
}

// ---------------------------------------------------------------------------
// the forecast side's view of a handle
// ---------------------------------------------------------------------------
// All a forecast entry point may use of a handle.  forecast_view (bnf_api.hip) builds it from the handle at call time,
// so there is no second copy of the state to go stale; a NULL handle gives bound = false, which every entry point
// refuses as "not bound" the way it refused !h || !h->bound.
struct Forecast {
  bool bound;          // bnf_bind has been called
  int32_t device;      // cfg.device
  int32_t obs_model;   // cfg.obs_model, BNF_OBS_*
  hipStream_t stream;
  float* qscratch;     // quantile partials: 2*1024*2 + 2 floats
};
BNF_HIDDEN Forecast forecast_view(const bnf_handle* h);
