// bnf_totals.h -- summaries and proper scores of an ensemble of sample paths on the device (bnf_sample_summaries,
// bnf_sample_energy_score): the counterpart, for the group totals bnf_predictive_group_sums writes, of what
// bnf_predictive_scores / bnf_count_rps are for the per-row marginals.  Input x (S, G) f64 row-major: S sample paths of G
// columns (group totals), and the observed totals y (G,) f64.  Everything is f64; no floating-point atomics; every sum is
// in an order the shapes fix, so two calls give the same bits.
//
// k_sample_summaries: per column c the S values sorted ascending in LDS, and from the sorted column
//   mean[c]      (1 / S) sum_i x_(i)
//   quant[j][c]  numpy's default ('linear') rule: h = (S - 1) q_j, x_(floor h) + (h - floor h) (x_(floor h + 1) - x_(floor h));
//                floor h and h - floor h are formed on the host in f64 (SummaryQ); h an integer gives x_(h) itself
//   pit[0][c], pit[1][c]   #{x_s <= y_c} / S and #{x_s < y_c} / S (totals of counts tie often)
//   crps[c]      (1 / S) sum_s |x_s - y_c| - (1 / S^2) sum_{i = 1..S} (2 i - S - 1) x_(i): the ensemble CRPS
//                E|X - y| - E|X - X'| / 2 as a V-statistic in its sorted form, evaluated on d_(i) = x_(i) - y_c (the second
//                sum is shift invariant: its coefficients add to 0), so that a total of 1e9 with a spread of 10 loses nothing
//   A column whose y_c is NaN or infinite gives NaN in crps and pit; a column holding a NaN sample gives NaN everywhere.
//   One workgroup sorts a slab of C adjacent columns (C * P <= 16,384 doubles, P = S rounded up to a power of two, C <= 8 a
//   power of two): the load then reads C * 8 contiguous bytes per sample path instead of 8.  The columns sit one after the
//   other in LDS, padded to P with +inf, and ONE bitonic network runs over all of them (C * P / 2 compare-exchanges per
//   stage, a barrier between stages; a column with a NaN sample does not come out sorted, but a compare-exchange only ever
//   permutes, and that column is reported NaN from a flag set at the load).  LDS is dynamic, 8 * C * P bytes <= 128 KiB.
//   Every LDS cell read has been written by this kernel: all C * P cells are filled (data, or +inf) before the first stage.
//   The sums: thread t adds the elements t, t + T, t + 2 T, ... in that order, the wave butterfly, then the waves in order.
//
// k_energy_first / k_energy_pairs / k_energy_finish: the energy score of the joint paths,
//   ES = (1 / S) sum_s |X_s - y|_2 - (1 / (2 S^2)) sum_{s,t} |X_s - X_t|_2,
//   the norms over the columns whose y_c is finite (none: NaN).  The pair sum costs S^2 G / 2 differences: the S x S pairs
//   are cut into tiles of 64 x 64 paths, only the tiles on and above the diagonal run (s < t; the sum is doubled, the
//   diagonal is 0), and the columns stream through LDS in chunks of 32, skipped columns as zeros on both sides.  Every
//   distance is sum_c (a_c - b_c)^2 from direct differences, columns in order, in f64 (the Gram form |a|^2 + |b|^2 - 2 a.b
//   cancels for paths that are close, which is exactly where the second term matters).  A thread owns 4 x 4 pairs (rows
//   ty + 16 i against rows tx + 16 j: the A reads of a wave are 4 broadcasts, the B reads 16 consecutive doubles; the
//   chunk is stored [column][path] with a pitch of 65 doubles so that the staging writes spread over the banks).  Each tile
//   writes ONE partial sum to work[S + tile], k_energy_first writes |X_s - y| to work[s], k_energy_finish adds both lists
//   in a fixed order.  work holds energy_work_doubles(S) doubles (include/bnf.h has the formula).
#pragma once

#include "bnf_sampling.h"

namespace bnf {

constexpr int kSumMaxSamples = BNF_SUMMARY_MAX_SAMPLES;
constexpr int kSumMaxQ = BNF_SUMMARY_MAX_QUANTILES;
constexpr int kSumMaxCols = 8;                      // columns per workgroup at most
constexpr int kSumMaxWaves = 16;
static_assert((kSumMaxSamples & (kSumMaxSamples - 1)) == 0, "the cap is a power of two: it is the padded length itself");
static_assert(sizeof(double) * kSumMaxSamples + 1024 <= 160 * 1024, "LDS per workgroup");

struct SummaryQ {                                   // the quantile levels, by value: floor((S - 1) q) and the fraction
  int32_t n;
  int32_t lo[kSumMaxQ];
  double frac[kSumMaxQ];
};

__device__ __forceinline__ bool totals_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN

// blockDim.x a multiple of 64, at most 1,024.  P a power of two >= S, C a power of two, C * P <= kSumMaxSamples.
__global__ __launch_bounds__(1024) void k_sample_summaries(const double* __restrict__ x, int32_t S, int64_t G, int32_t P,
                                                           int32_t C, const double* __restrict__ y, SummaryQ q,
                                                           double* __restrict__ mean, double* __restrict__ quant,
                                                           double* __restrict__ crps, double* __restrict__ pit) {
  extern __shared__ __attribute__((aligned(16))) double tot_sm[];
  __shared__ double red[kSumMaxWaves * 5];
  __shared__ int32_t has_nan[kSumMaxCols];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int64_t c0 = (int64_t)blockIdx.x * C;
  const int lc = __ffs(C) - 1, lp = __ffs(P) - 1;
  if (tid < kSumMaxCols) has_nan[tid] = 0;
  __syncthreads();
  for (int e = tid; e < (P << lc); e += nt) {         // (path, column of the slab): the slab's C columns are contiguous
    const int s = e >> lc, j = e & (C - 1);
    double v = INFINITY;
    if (s < S && c0 + j < G) {
      v = x[(int64_t)s * G + c0 + j];
      if (v != v) has_nan[j] = 1;
    }
    tot_sm[(j << lp) + s] = v;
  }
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int i = tid; i < (P << lc) >> 1; i += nt) {
        const int col = i >> (lp - 1), ii = i & ((P >> 1) - 1);
        const int lo = ((ii & ~(j - 1)) << 1) | (ii & (j - 1));
        const int hi = lo | j;
        double* b = tot_sm + (col << lp);
        const double u = b[lo], w = b[hi];
        if ((u > w) == ((lo & k) == 0)) { b[lo] = w; b[hi] = u; }
      }
    }
  }
  __syncthreads();

  const double nan_ = __builtin_nan("");
  const double dS = (double)S;
  for (int j = 0; j < C && c0 + j < G; ++j) {
    const int64_t c = c0 + j;
    const double* b = tot_sm + (j << lp);
    const double yv = y ? y[c] : nan_;
    const bool have = totals_finite(yv);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, n_le = 0.0, n_lt = 0.0;
    for (int i = tid; i < S; i += nt) {
      const double v = b[i];
      s0 += v;
      if (have) {
        const double d = v - yv;
        s1 += fabs(d);
        s2 += (double)(2 * i - S + 1) * d;             // 2 (i + 1) - S - 1
        n_le += v <= yv ? 1.0 : 0.0;
        n_lt += v < yv ? 1.0 : 0.0;
      }
    }
    s0 = wave_sum_f64(s0); s1 = wave_sum_f64(s1); s2 = wave_sum_f64(s2);
    n_le = wave_sum_f64(n_le); n_lt = wave_sum_f64(n_lt);
    if ((tid & 63) == 0) {
      double* r = red + (tid >> 6) * 5;
      r[0] = s0; r[1] = s1; r[2] = s2; r[3] = n_le; r[4] = n_lt;
    }
    __syncthreads();
    if (tid == 0) {
      double t[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
      for (int w = 0; w < (nt >> 6); ++w)
#pragma unroll
        for (int k = 0; k < 5; ++k) t[k] += red[w * 5 + k];
      const bool bad = has_nan[j] != 0;
      if (mean) mean[c] = bad ? nan_ : t[0] / dS;
      const bool scored = have && !bad;
      if (crps) crps[c] = scored ? t[1] / dS - t[2] / (dS * dS) : nan_;
      if (pit) {
        pit[c] = scored ? t[3] / dS : nan_;
        pit[G + c] = scored ? t[4] / dS : nan_;
      }
      for (int k = 0; k < q.n; ++k) {
        const int lo = q.lo[k];
        const double f = q.frac[k];
        double v = b[lo];
        if (f > 0.0) v = v + f * (b[lo + 1] - v);      // f > 0 only for lo < S - 1
        quant[(int64_t)k * G + c] = bad ? nan_ : v;
      }
    }
    __syncthreads();                                   // the next column overwrites red
  }
}

// ---------------------------------------------------------------------------------------------------------------------
constexpr int kEsTile = BNF_ENERGY_SAMPLE_TILE;     // paths per side of a pair tile
constexpr int kEsCols = 32;                         // columns per LDS chunk
constexpr int kEsPitch = kEsTile + 1;
static_assert(kEsTile == 64, "16 x 16 threads of 4 x 4 pairs");

constexpr int64_t energy_tiles(int64_t S) { return (S + kEsTile - 1) / kEsTile; }
constexpr int64_t energy_work_doubles(int64_t S) { return S + energy_tiles(S) * (energy_tiles(S) + 1) / 2; }

// work[s] = |X_s - y|_2 over the columns with a finite y: one workgroup per path, the columns strided over the threads
__global__ __launch_bounds__(256) void k_energy_first(const double* __restrict__ x, int64_t G, const double* __restrict__ y,
                                                      double* __restrict__ work) {
  __shared__ double wsum[4];
  const int tid = threadIdx.x;
  const double* row = x + (int64_t)blockIdx.x * G;
  double acc = 0.0;
  for (int64_t c = tid; c < G; c += 256) {
    const double yv = y[c];
    if (totals_finite(yv)) {
      const double d = row[c] - yv;
      acc = fma(d, d, acc);
    }
  }
  acc = wave_sum_f64(acc);
  if ((tid & 63) == 0) wsum[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) work[blockIdx.x] = sqrt(((wsum[0] + wsum[1]) + wsum[2]) + wsum[3]);
}

// grid (nT, nT): tile (ti = blockIdx.y, tj = blockIdx.x), the tiles below the diagonal leave at once.
// work[S + ti nT - ti (ti - 1) / 2 + (tj - ti)] = sum over the pairs s < t of the tile of |X_s - X_t|_2
__global__ __launch_bounds__(256) void k_energy_pairs(const double* __restrict__ x, int64_t S, int64_t G,
                                                      const double* __restrict__ y, double* __restrict__ work) {
  const int64_t ti = blockIdx.y, tj = blockIdx.x, nT = gridDim.x;
  if (tj < ti) return;
  __shared__ __attribute__((aligned(16))) double sa_[kEsCols * kEsPitch];
  __shared__ __attribute__((aligned(16))) double sb_[kEsCols * kEsPitch];
  __shared__ double wsum[4];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int lcol = tid & (kEsCols - 1), lrow = tid >> 5;          // staging: 32 columns x 8 paths per pass
  const int64_t a0 = ti * kEsTile, b0 = tj * kEsTile;
  double acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;

  for (int64_t cb = 0; cb < G; cb += kEsCols) {
    __syncthreads();                                   // the previous chunk's reads are done
    const int64_t c = cb + lcol;
    const bool cok = c < G && totals_finite(y[c < G ? c : 0]);
#pragma unroll
    for (int p = 0; p < kEsTile / 8; ++p) {
      const int r = lrow + 8 * p;
      const int64_t ra = a0 + r, rb = b0 + r;
      sa_[lcol * kEsPitch + r] = (cok && ra < S) ? x[ra * G + c] : 0.0;
      sb_[lcol * kEsPitch + r] = (cok && rb < S) ? x[rb * G + c] : 0.0;
    }
    __syncthreads();
#pragma unroll 4
    for (int cc = 0; cc < kEsCols; ++cc) {
      double av[4], bv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        av[i] = sa_[cc * kEsPitch + ty + 16 * i];
        bv[i] = sb_[cc * kEsPitch + tx + 16 * i];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double d = av[i] - bv[j];
          acc[i][j] = fma(d, d, acc[i][j]);
        }
    }
  }
  double t = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t ra = a0 + ty + 16 * i, rb = b0 + tx + 16 * j;
      t += (ra < rb && rb < S) ? sqrt(acc[i][j]) : 0.0;
    }
  t = wave_sum_f64(t);
  if ((tid & 63) == 0) wsum[tid >> 6] = t;
  __syncthreads();
  if (tid == 0) work[S + ti * nT - ti * (ti - 1) / 2 + (tj - ti)] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// one workgroup: ES = T1 / S - T2 / S^2 with T1 the sum of work[0 .. S), T2 the sum of the tile partials (each pair once:
// the 2 of the double sum and the 1 / 2 of the score cancel); thread t adds the entries t, t + 256, ... in that order
__global__ __launch_bounds__(256) void k_energy_finish(const double* __restrict__ work, int64_t S, int64_t n_tiles,
                                                       const double* __restrict__ y, int64_t G, double* __restrict__ out) {
  __shared__ double wsum[8];
  const int tid = threadIdx.x;
  double t1 = 0.0, t2 = 0.0;
  int any = 0;
  for (int64_t i = tid; i < S; i += 256) t1 += work[i];
  for (int64_t i = tid; i < n_tiles; i += 256) t2 += work[S + i];
  for (int64_t c = tid; c < G; c += 256) any |= totals_finite(y[c]) ? 1 : 0;
  any = __syncthreads_or(any);
  t1 = wave_sum_f64(t1);
  t2 = wave_sum_f64(t2);
  if ((tid & 63) == 0) { wsum[tid >> 6] = t1; wsum[4 + (tid >> 6)] = t2; }
  __syncthreads();
  if (tid == 0) {
    const double a = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3], b = ((wsum[4] + wsum[5]) + wsum[6]) + wsum[7];
    const double dS = (double)S;
    out[0] = any ? a / dS - b / (dS * dS) : __builtin_nan("");
  }
}

}  // namespace bnf
