// bnf_bands.h -- SIMULTANEOUS bands of an ensemble of sample paths (bnf_sample_depths, bnf_depth_levels,
// bnf_sample_envelope): the rank envelope of Myllymaki et al. 2017 ("Global envelope tests"), which holds a whole path
// with a given probability where the quantiles of bnf_sample_summaries hold each column alone.  Input x (S, C) f64
// row-major: S sample paths of C columns (table rows, or positions of a running-total curve), col_group (C,) int32 the
// group of every column (an entry outside [0, G) takes no part).  Integers throughout: no floating-point atomics, no
// floating-point sums, every ratio ONE f64 division of a count by (double)S; two calls give the same bits.
//
// The order is the total order of rank_key (bnf_ranking.h): -0.0 == +0.0, infinities of one sign tie.
//   d[s][c]   = min(#{t : x_tc <= x_sc}, #{t : x_tc >= x_sc}) - 1     in [0, S - 1]; s counts itself.  A column that
//               holds a NaN sample gives -1 to every path
//   D[s][g]   = min of d[s][c] over the columns of g
//   band k at a column = [x_(k), x_(S-1-k)] of the column sorted ascending, 0-indexed: path s lies inside band k at
//               every column of g exactly when D[s][g] >= k
//   od[c]     = min(#{t : x_tc <= y_c}, #{t : x_tc >= y_c}) - 1       in [-1, S - 1] for an observed y_c (not NaN); -1
//               in a column with a NaN sample.  OD[g] = min over the columns of g whose y_c is not NaN
//
// k_sample_depths / k_sample_envelope: one workgroup sorts a slab of W adjacent columns (W * P <= 16,384 keys, P = S
//   rounded up to a power of two, W <= 8 a power of two -- the slab layout of k_sample_summaries: a path's loads are W * 8
//   contiguous bytes).  The keys of a column sit one after the other in LDS, padded to P with ~0, which is above every
//   real key (+inf is 0xfff0...), and ONE bitonic network runs over all of them.  LDS is dynamic, 8 * W * P bytes
//   <= 128 KiB; all W * P cells are written before the first stage: every LDS cell read has been written by this kernel.
//   A column past the matrix, or one that takes no part, is all padding.
//   depths: thread s walks the W columns of path s; per column two binary searches over the cells 0 .. S - 1 ONLY (the
//   padding is neither a tie nor "above", as in k_sample_ranks): lb = the first cell >= key, ub = the first cell > key,
//   d = min(ub, S - lb) - 1.  Adjacent columns of one group are folded in registers; every change of group is one
//   integer atomicMin into depth[s][g], which the caller has filled with BNF_DEPTH_NONE: calls over column chunks, or
//   over several curves, accumulate into one joint depth whatever their order (min is associative and commutative).
//   W S log^2 P / 2 compare-exchanges and 2 W S log S probes per slab.
//   envelope: lower[j][c] = x_(k), upper[j][c] = x_(S-1-k) with k = level[j][group of c], the key turned back into
//   its value (a -0.0 comes back as +0.0); NaN for k outside [0, S - 1], a column that takes no part, and one holding a
//   NaN sample.
//
// k_depth_levels: one workgroup per group.  A histogram of D + 1 over S + 1 bins in LDS (dynamic, 4 (S + 1) bytes
//   <= 64 KiB + 4; zeroed here, filled with integer LDS atomics), a suffix scan over the bins (each of the 256 threads
//   owns a run of adjacent bins), after which ge(k) = #{s : D_sg >= k} is bin k + 1 and every output is a lookup:
//     level[i][g]    the largest k with ge(k) >= need_i           (the need_i-th largest of D[:, g]; ge(-1) = S)
//     achieved[i][g] ge(level) / S
//     joint[i][g]    ge(k_query_i) / S                             (k <= -1: 1; k >= S: 0)
//     obs_pit[0][g]  #{D <= OD} / S = (S - ge(OD + 1)) / S,  obs_pit[1][g] = #{D < OD} / S = (S - ge(OD)) / S
//   A depth outside [-1, S - 1] (BNF_DEPTH_NONE: no column took part; or an input that is not ours) is never turned
//   into a bin index: it sets a flag, and the group reports level -1 and NaN ratios.  A group poisoned by a NaN column
//   has every depth at -1: level -1, achieved 1.  An OD outside [-1, S - 1] gives a NaN obs_pit.
#pragma once

#include "bnf_ranking.h"
#include "bnf_totals.h"

namespace bnf {

constexpr int kBandMaxLevels = BNF_BAND_MAX_LEVELS;
constexpr int32_t kDepthNone = BNF_DEPTH_NONE;
constexpr int kBandThreads = 256;                   // k_depth_levels
static_assert(sizeof(uint64_t) * kSumMaxSamples <= 128 * 1024, "LDS per workgroup: the sorted slab");
static_assert(sizeof(int32_t) * (kSumMaxSamples + 1) + 2048 <= 160 * 1024, "LDS per workgroup: the histogram");

struct BandLevels {                                 // need and k_query, by value
  int32_t n_cov, n_query;
  int32_t need[kBandMaxLevels];
  int32_t k_query[kBandMaxLevels];
};

// the value of a key of rank_key (never called on the key of a NaN, 0, nor on the padding)
__device__ __forceinline__ double rank_unkey(uint64_t key) {
  const uint64_t b = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
  return __longlong_as_double((long long)b);
}

// The slab of W columns from c0 on as sorted keys: sm[(j << lp) + i], i = 0 .. S - 1 ascending, then padding.
// has_nan[j] = 1 for a column holding a NaN sample (its keys are sorted all the same: NaN is the key 0).
__device__ __forceinline__ void bands_sort_slab(const double* __restrict__ x, int32_t S, int64_t n_cols, int32_t P,
                                                int32_t W, int64_t c0, const int32_t* __restrict__ col_group,
                                                int32_t G, uint64_t* __restrict__ sm, int32_t* __restrict__ has_nan) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int lw = __ffs(W) - 1, lp = __ffs(P) - 1;
  if (tid < kSumMaxCols) has_nan[tid] = 0;
  __syncthreads();
  for (int e = tid; e < (P << lw); e += nt) {         // (path, column of the slab): the slab's W columns are contiguous
    const int s = e >> lw, j = e & (W - 1);
    uint64_t key = kRankPad;
    if (s < S && c0 + j < n_cols) {
      const int32_t g = col_group[c0 + j];
      if (g >= 0 && g < G) {
        const double v = x[(int64_t)s * n_cols + c0 + j];
        if (v != v) has_nan[j] = 1;
        key = rank_key(v);
      }
    }
    sm[(j << lp) + s] = key;
  }
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int i = tid; i < (P << lw) >> 1; i += nt) {
        const int col = i >> (lp - 1), ii = i & ((P >> 1) - 1);
        const int lo = ((ii & ~(j - 1)) << 1) | (ii & (j - 1));
        const int hi = lo | j;
        uint64_t* b = sm + (col << lp);
        const uint64_t u = b[lo], w = b[hi];
        if ((u > w) == ((lo & k) == 0)) { b[lo] = w; b[hi] = u; }
      }
    }
  }
  __syncthreads();
}

// min(#{cells <= key}, #{cells >= key}) - 1 over the sorted cells b[0 .. S)
__device__ __forceinline__ int32_t bands_depth_of(const uint64_t* __restrict__ b, int32_t S, uint64_t key) {
  int lo = 0, hi = S;                                  // the first cell >= key
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (b[mid] < key) lo = mid + 1; else hi = mid;
  }
  const int lb = lo;
  hi = S;                                              // the first cell > key: at or past lb
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (b[mid] <= key) lo = mid + 1; else hi = mid;
  }
  const int n_le = lo, n_ge = S - lb;
  return (n_le < n_ge ? n_le : n_ge) - 1;
}

// blockDim.x a multiple of 64, at most 1,024.  P a power of two >= S, W a power of two <= kSumMaxCols,
// W * P <= kSumMaxSamples; 8 W P bytes of dynamic LDS.  grid = ceil(n_cols / W).
__global__ __launch_bounds__(1024) void k_sample_depths(const double* __restrict__ x, int32_t S, int64_t n_cols, int32_t P,
                                                        int32_t W, const int32_t* __restrict__ col_group, int32_t G,
                                                        const double* __restrict__ y, int32_t* __restrict__ depth,
                                                        int32_t* __restrict__ obs_depth) {
  extern __shared__ __attribute__((aligned(16))) uint64_t band_sm[];
  __shared__ int32_t has_nan[kSumMaxCols];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int64_t c0 = (int64_t)blockIdx.x * W;
  const int lp = __ffs(P) - 1;
  bands_sort_slab(x, S, n_cols, P, W, c0, col_group, G, band_sm, has_nan);

  for (int s = tid; s < S; s += nt) {
    const double* row = x + (int64_t)s * n_cols;
    int32_t cur_g = -1, cur_d = kDepthNone;
    for (int j = 0; j < W && c0 + j < n_cols; ++j) {
      const int32_t g = col_group[c0 + j];
      if (g < 0 || g >= G) continue;
      // the column's own key is formed again from x (the same load as at the fill: the same bits)
      const int32_t d = has_nan[j] ? -1 : bands_depth_of(band_sm + (j << lp), S, rank_key(row[c0 + j]));
      if (g != cur_g) {
        if (cur_g >= 0) atomicMin(depth + (int64_t)s * G + cur_g, cur_d);
        cur_g = g;
        cur_d = d;
      } else if (d < cur_d) {
        cur_d = d;
      }
    }
    if (cur_g >= 0) atomicMin(depth + (int64_t)s * G + cur_g, cur_d);
  }
  if (y && tid < W && c0 + tid < n_cols) {
    const int32_t g = col_group[c0 + tid];
    const double yv = y[c0 + tid];
    if (g >= 0 && g < G && yv == yv)
      atomicMin(obs_depth + g, has_nan[tid] ? -1 : bands_depth_of(band_sm + (tid << lp), S, rank_key(yv)));
  }
}

// the launch of k_sample_depths; level (n_levels, G) int32, lower / upper (n_levels, n_cols) f64
__global__ __launch_bounds__(1024) void k_sample_envelope(const double* __restrict__ x, int32_t S, int64_t n_cols,
                                                          int32_t P, int32_t W, const int32_t* __restrict__ col_group,
                                                          int32_t G, const int32_t* __restrict__ level, int32_t n_levels,
                                                          double* __restrict__ lower, double* __restrict__ upper) {
  extern __shared__ __attribute__((aligned(16))) uint64_t band_sm[];
  __shared__ int32_t has_nan[kSumMaxCols];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int64_t c0 = (int64_t)blockIdx.x * W;
  const int lw = __ffs(W) - 1, lp = __ffs(P) - 1;
  bands_sort_slab(x, S, n_cols, P, W, c0, col_group, G, band_sm, has_nan);

  const double nan_ = __builtin_nan("");
  for (int e = tid; e < (n_levels << lw); e += nt) {
    const int jl = e >> lw, j = e & (W - 1);
    const int64_t c = c0 + j;
    if (c >= n_cols) continue;
    const int32_t g = col_group[c];
    double lo = nan_, hi = nan_;
    if (g >= 0 && g < G && !has_nan[j]) {
      const int32_t k = level[(int64_t)jl * G + g];
      if (k >= 0 && k <= S - 1) {
        lo = rank_unkey(band_sm[(j << lp) + k]);
        hi = rank_unkey(band_sm[(j << lp) + (S - 1 - k)]);
      }
    }
    lower[(int64_t)jl * n_cols + c] = lo;
    upper[(int64_t)jl * n_cols + c] = hi;
  }
}

// grid = G, kBandThreads threads; 4 (S + 1) bytes of dynamic LDS
__global__ __launch_bounds__(kBandThreads) void k_depth_levels(const int32_t* __restrict__ depth, int32_t S, int32_t G,
                                                               BandLevels q, const int32_t* __restrict__ obs_depth,
                                                               int32_t* __restrict__ level, double* __restrict__ achieved,
                                                               double* __restrict__ joint, double* __restrict__ obs_pit) {
  extern __shared__ __attribute__((aligned(16))) int32_t band_hist[];       // S + 1 bins: bin b counts D = b - 1
  __shared__ int32_t part[kBandThreads];
  const int tid = threadIdx.x;
  const int32_t g = blockIdx.x;
  const int n_bins = S + 1;
  for (int i = tid; i < n_bins; i += kBandThreads) band_hist[i] = 0;
  __syncthreads();
  int bad = 0;
  for (int s = tid; s < S; s += kBandThreads) {
    const int32_t d = depth[(int64_t)s * G + g];
    if (d < -1 || d > S - 1) bad = 1;                  // never a bin index
    else atomicAdd(&band_hist[d + 1], 1);
  }
  bad = __syncthreads_or(bad);
  // suffix scan: thread t owns the bins [t * run, (t + 1) * run)
  const int run = (n_bins + kBandThreads - 1) / kBandThreads;
  const int b0 = tid * run, b1 = b0 + run < n_bins ? b0 + run : n_bins;
  int32_t sum = 0;
  for (int i = b0; i < b1; ++i) sum += band_hist[i];
  part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    int32_t acc = 0;
    for (int t = kBandThreads - 1; t >= 0; --t) { const int32_t v = part[t]; part[t] = acc; acc += v; }   // the bins after t's
  }
  __syncthreads();
  int32_t acc = part[tid];
  for (int i = b1 - 1; i >= b0; --i) { acc += band_hist[i]; band_hist[i] = acc; }
  __syncthreads();
  // band_hist[b] = #{D + 1 >= b}: ge(k) = band_hist[k + 1] for k in [-1, S - 1]

  const double nan_ = __builtin_nan("");
  const double dS = (double)S;
  if (tid < q.n_cov) {
    int32_t k = -1;
    double a = nan_;
    if (!bad) {
      const int32_t need = q.need[tid];
      int lo = 0, hi = S;                              // the largest bin b in [0, S] with band_hist[b] >= need; bin 0 holds S
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (band_hist[mid] >= need) lo = mid; else hi = mid - 1;
      }
      k = lo - 1;
      a = (double)band_hist[lo] / dS;
    }
    if (level) level[(int64_t)tid * G + g] = k;
    if (achieved) achieved[(int64_t)tid * G + g] = a;
  }
  if (joint && tid < q.n_query) {
    const int32_t k = q.k_query[tid];
    const int32_t n = k <= -1 ? S : k > S - 1 ? 0 : band_hist[k + 1];
    joint[(int64_t)tid * G + g] = bad ? nan_ : (double)n / dS;
  }
  if (obs_pit && tid == 0) {
    const int32_t od = obs_depth[g];
    double p_le = nan_, p_lt = nan_;
    if (!bad && od >= -1 && od <= S - 1) {
      const int32_t ge_next = od + 1 > S - 1 ? 0 : band_hist[od + 2];
      p_le = (double)(S - ge_next) / dS;
      p_lt = (double)(S - band_hist[od + 1]) / dS;
    }
    obs_pit[g] = p_le;
    obs_pit[(int64_t)G + g] = p_lt;
  }
}

}  // namespace bnf
