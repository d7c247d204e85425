// bnf_stacking.h -- stacking of predictive distributions on held-out rows (bnf_member_log_density /
// bnf_stacking_weights): simplex weights w over the M members that maximise the held-out log score
//       f(w) = (1 / n) sum_r log sum_m w_m p_m(y_r)                                      (Yao et al. 2018)
// where the forecasts of bnf_predictive_scores use w = 1 / M.  The optimiser is EM on the mixture weights,
//       g_m = (1 / n) sum_r p_m(y_r) / sum_k w_k p_k(y_r),       w_m <- w_m g_m      (sum_m w_m g_m = 1)
// which never leaves the simplex and never lowers f.  g is the gradient of f; f is concave, so for the optimum w*
//       f(w*) - f(w) <= sum_m w*_m g_m - 1 <= max_m g_m - 1 = gap
// a bound that is computed from the iterate alone: the loop stops on gap <= tol and reports the gap it stopped at.
//
//   k_member_log_density     L (M, R) f32, L[m][r] = score_log_density(y_r, loc[m][r], aux[m]) (bnf_scoring.h: the forms of
//                            the training loss); NaN in every member of a row whose y is not finite; -inf is a legal value.
//   k_stack_rows             block = tile of kStackTile rows (256 threads x 4 rows), two passes over the members:
//                              1: lse_r = log sum_m w_m exp(L_mr), running max and scaled sum; members with w_m = 0 or
//                                 L_mr = -inf add nothing
//                              2: exp(L_mr - lse_r), summed over the tile by the fixed tree (4 per thread, wave butterfly,
//                                 4 waves) -> partial[tile][m]; the tile's sum of lse_r and its row counts -> tile_stat
//                            A row is SCORED when none of its L is NaN and lse_r is finite; the other rows without a NaN
//                            (every weighted member at -inf) are DROPPED: left out of every sum, and counted.
//   k_stack_combine          ONE block: n, f, g_m (every member, zero weights included), gap; then either the stop (gap <=
//                            tol, the iteration budget spent, no scored row: sets the flag, writes info, leaves w alone) or
//                            the update w_m <- w_m g_m, renormalised.
//   k_stack_rows<true>       the final pass: lpd[r] = (float) lse_r at the returned weights; NaN rows NaN, dropped rows -inf.
// Both kernels of an iteration return at once when the flag is set, so the host may enqueue them in batches and look at
// the flag once per batch.
//
// Arithmetic: everything after L is f64, exp and log included.  Every sum is in an order the shapes fix (no floating-point
// atomics): two calls give the same bits.  Plain HIP C++.
#pragma once

#include "bnf_scoring.h"

namespace bnf {

constexpr int kStackTile = BNF_STACK_ROW_TILE;
constexpr int kStackRowsPerThread = 4;
constexpr int kStackState = BNF_STACK_STATE_DOUBLES;
static_assert(kStackTile == 256 * kStackRowsPerThread, "row tile = one block of 256 threads x 4 rows");
// state (kStackState doubles at the head of the work buffer)
enum : int { STACK_DONE = 0, STACK_ITERS = 1, STACK_F0 = 2, STACK_HAVE_F0 = 3 };
// tile_stat (n_tiles, 3): sum of lse_r over the scored rows, scored rows, dropped rows
enum : int { STACK_T_LSE = 0, STACK_T_SCORED = 1, STACK_T_DROPPED = 2 };

template <int OBS>
__global__ __launch_bounds__(256) void k_member_log_density(const float* __restrict__ loc, const float* __restrict__ aux,
                                                            int32_t M, int64_t R, const float* __restrict__ y,
                                                            float* __restrict__ out) {
  const int64_t base = (int64_t)blockIdx.x * kStackTile + threadIdx.x;
  float yv[kStackRowsPerThread];
  bool in[kStackRowsPerThread], ok[kStackRowsPerThread];
#pragma unroll
  for (int i = 0; i < kStackRowsPerThread; ++i) {
    const int64_t r = base + i * 256;
    in[i] = r < R;
    yv[i] = in[i] ? y[r] : 0.f;
    ok[i] = in[i] && score_finite(yv[i]);
  }
  for (int32_t m = blockIdx.y; m < M; m += gridDim.y) {
    const float a0 = aux[m * 3], a1 = aux[m * 3 + 1], a2 = aux[m * 3 + 2];
    const float* lrow = loc + (int64_t)m * R;
    float* orow = out + (int64_t)m * R;
#pragma unroll 1
    for (int i = 0; i < kStackRowsPerThread; ++i) {
      const int64_t r = base + i * 256;
      if (in[i]) orow[r] = ok[i] ? score_log_density<OBS>(yv[i], lrow[r], a0, a1, a2) : __builtin_nanf("");
    }
  }
}

// w (M,), *state = 0: the start of a call.  w_init == nullptr: uniform.
__global__ __launch_bounds__(256) void k_stack_init(const double* __restrict__ w_init, int32_t M, double* __restrict__ w,
                                                    double* __restrict__ state) {
  const int tid = threadIdx.x;
  const double u = 1.0 / (double)M;
  for (int32_t m = tid; m < M; m += 256) w[m] = w_init ? w_init[m] : u;
  if (tid < kStackState) state[tid] = 0.0;
}

// the sum of one value per thread over a block of 256, in a fixed order; every thread gets it.  `buf`: 4 doubles of LDS
__device__ __forceinline__ double stack_block_sum(double v, double* buf) {
  v = wave_sum_f64(v);
  __syncthreads();                                           // the previous use of buf has been read
  if ((threadIdx.x & 63) == 0) buf[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((buf[0] + buf[1]) + buf[2]) + buf[3];
}

__device__ __forceinline__ double stack_block_max(double v, double* buf) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) buf[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmax(fmax(buf[0], buf[1]), fmax(buf[2], buf[3]));
}

// grid (n_tiles).  FINAL = false: one iteration's row pass (partial (n_tiles, M), tile_stat (n_tiles, 3)).
// FINAL = true: lpd only.
template <bool FINAL>
__global__ __launch_bounds__(256) void k_stack_rows(const float* __restrict__ L, int32_t M, int64_t R,
                                                    const double* __restrict__ w, const double* __restrict__ state,
                                                    double* __restrict__ partial, double* __restrict__ tile_stat,
                                                    float* __restrict__ lpd) {
  __shared__ double wsum[2][4];
  __shared__ double red[4];
  if (!FINAL && state[STACK_DONE] != 0.0) return;            // the same in every thread
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * kStackTile + tid;
  bool in[kStackRowsPerThread], nan[kStackRowsPerThread];
  double mx[kStackRowsPerThread], s[kStackRowsPerThread];
#pragma unroll
  for (int i = 0; i < kStackRowsPerThread; ++i) {
    in[i] = base + i * 256 < R;
    nan[i] = false;
    mx[i] = -INFINITY;
    s[i] = 0.0;
  }
#pragma unroll 1
  for (int32_t m = 0; m < M; ++m) {
    const double wm = w[m];
    const float* lrow = L + (int64_t)m * R;
#pragma unroll
    for (int i = 0; i < kStackRowsPerThread; ++i) {
      if (!in[i]) continue;
      const double l = (double)lrow[base + i * 256];
      if (l != l) nan[i] = true;
      else if (wm > 0.0 && l > -INFINITY) {
        if (l <= mx[i]) s[i] += wm * exp(l - mx[i]);         // one exp either way: the maximum moves a few times per row
        else { s[i] = s[i] * exp(mx[i] - l) + wm; mx[i] = l; }   // mx = -inf: s = 0, exp(-inf) = 0
      }
    }
  }
  double lse[kStackRowsPerThread];
  bool scored[kStackRowsPerThread];
  double t_lse = 0.0, t_scored = 0.0, t_dropped = 0.0;
#pragma unroll
  for (int i = 0; i < kStackRowsPerThread; ++i) {
    lse[i] = mx[i] + log(s[i]);                              // nothing added: -inf + log 0 = -inf
    const bool live = in[i] && !nan[i];
    scored[i] = live && fabs(lse[i]) <= 1.7976931348623157e308;
    if (FINAL) {
      if (in[i]) lpd[base + i * 256] = nan[i] ? __builtin_nanf("") : (scored[i] ? (float)lse[i] : -INFINITY);
    } else {
      t_lse += scored[i] ? lse[i] : 0.0;
      t_scored += scored[i] ? 1.0 : 0.0;
      t_dropped += (live && !scored[i]) ? 1.0 : 0.0;
    }
  }
  if (FINAL) return;
  t_lse = stack_block_sum(t_lse, red);
  t_scored = stack_block_sum(t_scored, red);
  t_dropped = stack_block_sum(t_dropped, red);
  if (tid == 0) {
    double* ts = tile_stat + (int64_t)blockIdx.x * 3;
    ts[STACK_T_LSE] = t_lse;
    ts[STACK_T_SCORED] = t_scored;
    ts[STACK_T_DROPPED] = t_dropped;
  }
  double* prow = partial + (int64_t)blockIdx.x * M;
#pragma unroll 1
  for (int32_t m = 0; m < M; ++m) {
    const float* lrow = L + (int64_t)m * R;
    double v[kStackRowsPerThread];
#pragma unroll
    for (int i = 0; i < kStackRowsPerThread; ++i)
      v[i] = scored[i] ? exp((double)lrow[base + i * 256] - lse[i]) : 0.0;
    const double t = wave_sum_f64(((v[0] + v[1]) + v[2]) + v[3]);
    if ((tid & 63) == 0) wsum[m & 1][tid >> 6] = t;
    __syncthreads();                                         // one per member: member m + 1 writes the other half of wsum,
    if (tid == 0)                                            // and nobody reaches m + 2 before thread 0 has passed m + 1
      prow[m] = ((wsum[m & 1][0] + wsum[m & 1][1]) + wsum[m & 1][2]) + wsum[m & 1][3];
  }
}

// ONE block of 256.  info (5,): objective and gap at the returned weights, objective at the start, iterations, rows dropped.
__global__ __launch_bounds__(256) void k_stack_combine(const double* __restrict__ partial,
                                                       const double* __restrict__ tile_stat, int32_t M, int64_t n_tiles,
                                                       int64_t max_iter, double tol, double* __restrict__ w,
                                                       double* __restrict__ state, double* __restrict__ info) {
  __shared__ double red[4];
  if (state[STACK_DONE] != 0.0) return;                      // the same in every thread
  const int tid = threadIdx.x;
  double a = 0.0, b = 0.0, c = 0.0;
  for (int64_t j = tid; j < n_tiles; j += 256) {
    a += tile_stat[j * 3 + STACK_T_LSE];
    b += tile_stat[j * 3 + STACK_T_SCORED];
    c += tile_stat[j * 3 + STACK_T_DROPPED];
  }
  const double lse_sum = stack_block_sum(a, red);
  const double n = stack_block_sum(b, red);
  const double dropped = stack_block_sum(c, red);
  const double iters = state[STACK_ITERS];
  const double f = lse_sum / n;
  const double f0 = state[STACK_HAVE_F0] != 0.0 ? state[STACK_F0] : f;
  __syncthreads();                                           // every thread has read the state
  if (n == 0.0) {
    if (tid == 0) {
      const double nan = __builtin_nan("");
      info[0] = nan; info[1] = nan; info[2] = nan; info[3] = iters; info[4] = dropped;
      state[STACK_DONE] = 1.0;
    }
    return;
  }
  // g_m and w_m g_m of the members this thread owns (m = tid, tid + 256, ...); the tiles in order
  double gmax = -INFINITY, wg_sum = 0.0;
  for (int32_t m = tid; m < M; m += 256) {
    double g = 0.0;
    for (int64_t j = 0; j < n_tiles; ++j) g += partial[j * M + m];
    g /= n;
    gmax = fmax(gmax, g);
    wg_sum += w[m] * g;
  }
  const double gap = stack_block_max(gmax, red) - 1.0;
  if (gap <= tol || iters >= (double)max_iter) {
    if (tid == 0) {
      info[0] = f; info[1] = f0; info[2] = gap; info[3] = iters; info[4] = dropped;
      state[STACK_DONE] = 1.0;
    }
    return;
  }
  const double norm = stack_block_sum(wg_sum, red);          // 1 up to rounding
  for (int32_t m = tid; m < M; m += 256) {
    double g = 0.0;
    for (int64_t j = 0; j < n_tiles; ++j) g += partial[j * M + m];
    g /= n;
    w[m] = (w[m] * g) / norm;
  }
  if (tid == 0) {
    state[STACK_ITERS] = iters + 1.0;
    state[STACK_F0] = f0;
    state[STACK_HAVE_F0] = 1.0;
  }
}

}  // namespace bnf
