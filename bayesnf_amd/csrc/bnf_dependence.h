// bnf_dependence.h -- how the columns of an ensemble of sample paths move together (bnf_sample_pair_moments): the
// predictive covariance and the variogram of every pair of columns, and the variogram score of the joint forecast
// (Scheuerer & Hamill 2015), the companion of the energy score of bnf_totals.h that does see a wrong correlation
// structure.  Input x (S, G) f64 row-major: S sample paths of G columns (the group totals bnf_predictive_group_sums
// writes), optionally the observed totals y (G,) f64 and pair weights pair_w (G, G) f64.  Everything is f64; no
// floating-point atomics; every sum is in an order the shapes fix, so two calls give the same bits.
//
// k_column_means: m_c = (1 / S) sum_s x_sc.  A workgroup owns 32 adjacent columns (a path's 32 values are 256 contiguous
//   bytes); thread (column, r) adds the paths r, r + 8, r + 16, ... in that order, the 8 partial sums of a column are added
//   in the order of r: the order depends on S alone.
//
// k_pair_moments<P, COV, VAR>: per pair of columns (i, j)
//   cov[i][j]   = (1 / S) sum_s (x_si - m_i) (x_sj - m_j)   centred products (never E[xy] - E[x] E[y]: a total of 1e9 with
//                 a spread of 10 loses nothing); the divisor is S, the ensemble's own moment: np.cov(x.T, bias=True)
//   vario[i][j] = (1 / S) sum_s |x_si - x_sj|^p             P = 0: sqrt(fabs d), 1: fabs d, 2: d * d.  There is no pow.
//   The G x G pairs are cut into tiles of 64 x 64 columns, only the tiles on and above the diagonal run, and the paths stream
//   through LDS in chunks of 32: the (chunk x tile) block of x is 64 contiguous doubles per path, so it is stored as it
//   lies, [path][column], once for the tile's rows (A) and once for its columns (B): 2 x 16 KiB, raw values -- the
//   variogram needs raw differences, the covariance centred ones, and the 8 means a thread needs stay in registers.  A
//   thread owns 4 x 4 pairs (columns ty + 16 i of A against tx + 16 j of B: the A reads of a wave are 4 broadcasts, the B
//   reads 16 consecutive doubles, the staging writes 64 consecutive doubles: no bank conflicts, no padding).  Every cell is
//   ONE sequential chain over s = 0 .. S - 1 (an fma per path, or an add for P < 2), so its bits depend on S and its two
//   columns only, not on G, on the tile it falls in or on the other columns of the call.  A ragged last chunk runs a
//   shorter loop (the LDS rows past it are neither written nor read); columns >= G are staged as zeros and their cells
//   dropped.  Every LDS cell read has been written by this kernel.
//   Only the cells i <= j are kept; each is written to [i][j] and [j][i], so both matrices are whole and bitwise symmetric
//   (the diagonal tile computes its lower half too and drops it).  vario[i][i] and the cell of two identical columns are
//   exactly 0 (every difference is).  A NaN sample makes its row and column NaN in both matrices by plain propagation.
//   With y (work != NULL), the tile adds  w_ij (|y_i - y_j|^p - vario_ij)^2  over its pairs i < j with y_i and y_j
//   finite -- w_ij = 1 or pair_w[i][j], read above the diagonal only -- thread cells in order, wave butterfly, waves in
//   order, and writes ONE partial sum to work[ti nT - ti (ti - 1) / 2 + (tj - ti)].  A scored column holding a NaN sample
//   makes the score NaN (also at w_ij = 0: the weight is a plain factor).  COV / VAR instantiate only the sums that are
//   asked for; the variogram's arithmetic is the same in every instantiation (contraction is off, every fma is written).
//
// k_vario_finish: one workgroup adds the partial sums, thread t the entries t, t + 256, ... in that order; fewer than two
//   finite y_c: NaN.
#pragma once

#include "bnf_sampling.h"
#include "bnf_totals.h"

namespace bnf {

constexpr int kDpTile = BNF_PAIR_COL_TILE;          // columns per side of a pair tile
constexpr int kDpChunk = BNF_PAIR_PATH_CHUNK;       // paths per LDS chunk
constexpr int kDpMeanCols = 32, kDpMeanLanes = 8;
static_assert(kDpTile == 64, "16 x 16 threads of 4 x 4 pairs; a staging pass is 4 paths of 64 columns");
static_assert(kDpChunk % 4 == 0, "a staging pass is 4 paths");
static_assert(2 * sizeof(double) * kDpChunk * kDpTile <= 40 * 1024, "four workgroups per CU");

constexpr int64_t pair_tiles(int64_t G) { return (G + kDpTile - 1) / kDpTile; }
constexpr int64_t pair_work_doubles(int64_t G) { return pair_tiles(G) * (pair_tiles(G) + 1) / 2; }

__global__ __launch_bounds__(256) void k_column_means(const double* __restrict__ x, int64_t S, int64_t G,
                                                      double* __restrict__ mean) {
  __shared__ double part[kDpMeanLanes][kDpMeanCols];
  const int tid = threadIdx.x, lc = tid & (kDpMeanCols - 1), lr = tid / kDpMeanCols;
  const int64_t c = (int64_t)blockIdx.x * kDpMeanCols + lc;
  double acc = 0.0;
  if (c < G)
    for (int64_t s = lr; s < S; s += kDpMeanLanes) acc += x[s * G + c];
  part[lr][lc] = acc;
  __syncthreads();
  if (lr == 0 && c < G) {
    double t = part[0][lc];
#pragma unroll
    for (int r = 1; r < kDpMeanLanes; ++r) t += part[r][lc];
    mean[c] = t / (double)S;
  }
}

// |d|^p in its three compiled forms
template <int P>
__device__ __forceinline__ double vario_term(double d) {
  if constexpr (P == 0) return sqrt(fabs(d));
  else if constexpr (P == 1) return fabs(d);
  else return d * d;
}

// one path of the chunk: a, b the path's rows of the two LDS images
template <int P, bool COV, bool VAR>
__device__ __forceinline__ void pair_step(const double* __restrict__ a, const double* __restrict__ b, int tx, int ty,
                                          const double (&ma)[4], const double (&mb)[4], double (&accc)[4][4],
                                          double (&accv)[4][4]) {
#pragma clang fp contract(off)
  double av[4], bv[4], ca[4], cb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    av[i] = a[ty + 16 * i];
    bv[i] = b[tx + 16 * i];
    if constexpr (COV) {
      ca[i] = av[i] - ma[i];
      cb[i] = bv[i] - mb[i];
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if constexpr (COV) accc[i][j] = fma(ca[i], cb[j], accc[i][j]);
      if constexpr (VAR) {
        const double d = av[i] - bv[j];
        if constexpr (P == 2) accv[i][j] = fma(d, d, accv[i][j]);
        else accv[i][j] = accv[i][j] + vario_term<P>(d);
      }
    }
}

// grid (nT, nT): tile (ti = blockIdx.y, tj = blockIdx.x), the tiles below the diagonal leave at once.  cov (COV) and mean
// (COV) are not NULL; vario, work (with y; pair_w optional) may be, VAR says that one of them is not.
template <int P, bool COV, bool VAR>
__global__ __launch_bounds__(256) void k_pair_moments(const double* __restrict__ x, int64_t S, int64_t G,
                                                      const double* __restrict__ mean, const double* __restrict__ y,
                                                      const double* __restrict__ pair_w, double* __restrict__ cov,
                                                      double* __restrict__ vario, double* __restrict__ work) {
  const int64_t ti = blockIdx.y, tj = blockIdx.x, nT = gridDim.x;
  if (tj < ti) return;
  __shared__ __attribute__((aligned(16))) double sa_[kDpChunk * kDpTile];
  __shared__ __attribute__((aligned(16))) double sb_[kDpChunk * kDpTile];
  __shared__ double wsum[4];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int lcol = tid & (kDpTile - 1), lrow = tid >> 6;          // staging: 4 paths x 64 columns per pass
  const int64_t a0 = ti * kDpTile, b0 = tj * kDpTile;
  const int64_t sca = a0 + lcol, scb = b0 + lcol;
  const bool oka = sca < G, okb = scb < G;
  double ma[4], mb[4], accc[4][4], accv[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t ci = a0 + ty + 16 * i, cj = b0 + tx + 16 * i;
    ma[i] = (COV && ci < G) ? mean[ci] : 0.0;
    mb[i] = (COV && cj < G) ? mean[cj] : 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) accc[i][j] = accv[i][j] = 0.0;
  }

  for (int64_t s0 = 0; s0 < S; s0 += kDpChunk) {
    const int n = S - s0 < kDpChunk ? (int)(S - s0) : kDpChunk;
    __syncthreads();                                   // the previous chunk's reads are done
#pragma unroll
    for (int p = 0; p < kDpChunk / 4; ++p) {
      const int r = lrow + 4 * p;
      if (r < n) {
        const double* row = x + (s0 + r) * G;
        sa_[r * kDpTile + lcol] = oka ? row[sca] : 0.0;
        sb_[r * kDpTile + lcol] = okb ? row[scb] : 0.0;
      }
    }
    __syncthreads();
    if (n == kDpChunk) {
#pragma unroll 4
      for (int ss = 0; ss < kDpChunk; ++ss)
        pair_step<P, COV, VAR>(sa_ + ss * kDpTile, sb_ + ss * kDpTile, tx, ty, ma, mb, accc, accv);
    } else {
      for (int ss = 0; ss < n; ++ss)
        pair_step<P, COV, VAR>(sa_ + ss * kDpTile, sb_ + ss * kDpTile, tx, ty, ma, mb, accc, accv);
    }
  }

  {
#pragma clang fp contract(off)
    const double dS = (double)S;
    const bool scoring = VAR && work != nullptr;
    double ya[4], yb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t ci = a0 + ty + 16 * i, cj = b0 + tx + 16 * i;
      ya[i] = (scoring && ci < G) ? y[ci] : __builtin_nan("");
      yb[i] = (scoring && cj < G) ? y[cj] : __builtin_nan("");
    }
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t ci = a0 + ty + 16 * i, cj = b0 + tx + 16 * j;
        if (cj >= G || ci > cj) continue;              // ci <= cj < G
        if constexpr (COV) {
          const double v = accc[i][j] / dS;
          cov[ci * G + cj] = v;
          cov[cj * G + ci] = v;
        }
        if constexpr (VAR) {
          const double v = accv[i][j] / dS;
          if (vario) {
            vario[ci * G + cj] = v;
            vario[cj * G + ci] = v;
          }
          if (scoring && ci < cj && totals_finite(ya[i]) && totals_finite(yb[j])) {
            const double e = vario_term<P>(ya[i] - yb[j]) - v;
            const double w = pair_w ? pair_w[ci * G + cj] : 1.0;
            t = fma(w, e * e, t);
          }
        }
      }
    if (scoring) {                                     // (uniform over the workgroup)
      t = wave_sum_f64(t);
      if ((tid & 63) == 0) wsum[tid >> 6] = t;
      __syncthreads();
      if (tid == 0) work[ti * nT - ti * (ti - 1) / 2 + (tj - ti)] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    }
  }
}

// one workgroup: out[0] = the sum of the n_tiles partial sums; NaN with fewer than two finite y_c
__global__ __launch_bounds__(256) void k_vario_finish(const double* __restrict__ work, int64_t n_tiles,
                                                      const double* __restrict__ y, int64_t G, double* __restrict__ out) {
  __shared__ double wsum[8];
  const int tid = threadIdx.x;
  double t = 0.0, n = 0.0;
  for (int64_t i = tid; i < n_tiles; i += 256) t += work[i];
  for (int64_t c = tid; c < G; c += 256) n += totals_finite(y[c]) ? 1.0 : 0.0;
  t = wave_sum_f64(t);
  n = wave_sum_f64(n);
  if ((tid & 63) == 0) { wsum[tid >> 6] = t; wsum[4 + (tid >> 6)] = n; }
  __syncthreads();
  if (tid == 0) {
    const double a = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3], cnt = ((wsum[4] + wsum[5]) + wsum[6]) + wsum[7];
    out[0] = cnt >= 2.0 ? a : __builtin_nan("");
  }
}

template <int P>
static void launch_pair_moments(hipStream_t stream, const double* x, int64_t S, int64_t G, const double* mean,
                                const double* y, const double* pair_w, double* cov, double* vario, double* work) {
  const int64_t nT = pair_tiles(G);
  const dim3 grid((unsigned)nT, (unsigned)nT), block(256);
  const bool var = vario || work;
  if (cov && var)
    hipLaunchKernelGGL((k_pair_moments<P, true, true>), grid, block, 0, stream, x, S, G, mean, y, pair_w, cov, vario, work);
  else if (cov)
    hipLaunchKernelGGL((k_pair_moments<P, true, false>), grid, block, 0, stream, x, S, G, mean, y, pair_w, cov, vario, work);
  else
    hipLaunchKernelGGL((k_pair_moments<P, false, true>), grid, block, 0, stream, x, S, G, mean, y, pair_w, cov, vario, work);
}

}  // namespace bnf
