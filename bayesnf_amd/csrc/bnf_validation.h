// bnf_validation.h -- held-out validation during a fit (bnf_validation_check): after a segment of bnf_train the caller
// scores the held-out rows (bnf_forward on a forward-only handle that reads the training parameters in place, then
// bnf_predictive_scores' member_ll) and this pair of kernels decides, per member and on the device, whether the check is
// the member's best so far, and keeps a snapshot of the parameters where it is.  No host round trip: the host never
// learns the decision while the fit runs.
//
//   k_validation_decide      one thread per member: score = member_ll[m] / (double)n_scored (one f64 division) into
//                            curve[m][check];
//                              check == 0: keep, whatever the score (NaN and -inf included: best_* are never read
//                                          uninitialised)
//                              check  > 0: keep = score > best || (isnan(best) && !isnan(score)) -- a tie keeps the
//                                          earlier epoch, a NaN never replaces a number, -inf never replaces -inf
//                            keep[m] = 0 / 1; where 1, best_score[m] = score and best_epoch[m] = epoch.
//   k_validation_copy        grid (ceil(P / kValCopyTile), members), launched AFTER the decide kernel on the same stream:
//                            every block reads keep[m] as the finished decide kernel left it (a decision taken inside the
//                            copy kernel would be read by blocks racing with its update) and, where it is 1, copies its
//                            tile of row m of the training parameters into row m of the snapshot as plain coalesced
//                            dwords (row m starts at byte m * P * 4, in general not 16-byte aligned: a wider copy would
//                            need head and tail handling).  Rows with keep[m] == 0 are not touched.  The copy is a pure
//                            HBM stream of at most 8 * members * P bytes.
//
// No floating-point atomics, no sum at all: two calls give the same bits.  Plain HIP C++.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace bnf {

constexpr int kValCopyPerThread = 4;
constexpr int kValCopyTile = 256 * kValCopyPerThread;   // dwords of one parameter row a block copies

__global__ __launch_bounds__(256) void k_validation_decide(const double* __restrict__ member_ll, int64_t n_scored,
                                                           int64_t epoch, int32_t check, int32_t n_checks, int32_t M,
                                                           double* __restrict__ curve, double* __restrict__ best_score,
                                                           int64_t* __restrict__ best_epoch, int32_t* __restrict__ keep) {
  const int32_t m = (int32_t)(blockIdx.x * 256 + threadIdx.x);
  if (m >= M) return;
  const double score = member_ll[m] / (double)n_scored;
  curve[(int64_t)m * n_checks + check] = score;
  bool k = true;
  if (check > 0) {
    const double best = best_score[m];
    k = score > best || (best != best && score == score);
  }
  keep[m] = k ? 1 : 0;
  if (k) {
    best_score[m] = score;
    best_epoch[m] = epoch;
  }
}

// params, best: (M, P) f32 read and written as raw dwords (a snapshot is the bits of the parameters)
__global__ __launch_bounds__(256) void k_validation_copy(const uint32_t* __restrict__ params, int64_t P, int32_t M,
                                                         const int32_t* __restrict__ keep, uint32_t* __restrict__ best) {
  const int64_t i0 = (int64_t)blockIdx.x * kValCopyTile + threadIdx.x;
  for (int32_t m = blockIdx.y; m < M; m += gridDim.y) {
    if (keep[m] == 0) continue;
    const uint32_t* src = params + (int64_t)m * P;
    uint32_t* dst = best + (int64_t)m * P;
    uint32_t v[kValCopyPerThread];
#pragma unroll
    for (int j = 0; j < kValCopyPerThread; ++j) {
      const int64_t i = i0 + j * 256;
      v[j] = i < P ? src[i] : 0u;
    }
#pragma unroll
    for (int j = 0; j < kValCopyPerThread; ++j) {
      const int64_t i = i0 + j * 256;
      if (i < P) dst[i] = v[j];
    }
  }
}

}  // namespace bnf
