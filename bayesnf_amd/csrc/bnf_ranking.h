// bnf_ranking.h -- how the columns of an ensemble of sample paths RANK against each other within a path
// (bnf_sample_ranks, bnf_rank_probabilities): "which groups are among the k largest", the question no marginal answers.
// Input x (S, G) f64 row-major: S sample paths of G columns (the group totals bnf_predictive_group_sums writes), optionally
// a per-column divisor scale (G,) f64 (a population: rank per capita).  Integer and f64 outputs; no floating-point atomics;
// every sum is in an order the shapes fix, so two calls give the same bits.
//
// k_sample_ranks: per path s the ranked values v_sg = x_sg / scale_g (a plain IEEE division; scale == NULL: v = x) and
//   above[s][g] = #{h : v_sh > v_sg}
//   ties[s][g]  = #{h : v_sh == v_sg}            g itself included: >= 1
//   rank[s][g]  = above + (ties + 1) / 2          the mid-rank, a multiple of 0.5; rank 1 is the largest value
//   Ties share their block of ranks equally; they are never broken by the column index (totals of counts tie all the
//   time).  The comparison is a total order: -0.0 == +0.0, +inf == +inf, NaN == NaN, and a NaN is below everything, -inf
//   included.  rank_key maps a value to a 64-bit key whose unsigned order is that order (NaN -> 0, a negative value ->
//   the complement of its bits, any other -> its bits with the sign bit set), so equal values have equal keys.
//   One workgroup handles one path and strides over the paths.  The G keys are sorted ascending in LDS by the bitonic
//   network of bnf_totals.h, padded to P (a power of two) with the key ~0, which is above every real key (the largest,
//   +inf, is 0xfff0...): after the sort the real keys are the cells 0 .. G - 1 and the padding G .. P - 1.  Every column
//   then makes two binary searches over the cells 0 .. G - 1 ONLY, so that the padding is neither a tie nor "above":
//   lb = the first cell >= key, ub = the first cell > key, ties = ub - lb, above = G - ub.  G log^2 G compare-exchanges
//   and 2 G log G probes per path.  LDS is dynamic, 8 P bytes <= 128 KiB; all P cells are written before the first stage:
//   every LDS cell read has been written by this kernel.  The integers depend on the path's values alone, not on the
//   launch geometry.
//
// k_rank_probabilities: out[k - 1][g] = (1 / S) sum_s [above_sg < k <= above_sg + ties_sg] / ties_sg, k = 1 .. K: the
//   probability that column g takes rank slot k, a tied block handing each of its slots to its members in equal shares.
//   A workgroup owns a slab of 64 adjacent columns (the reads of a path are 256 contiguous bytes per matrix) and 16
//   consecutive k; the paths stream through LDS 32 at a time as (above + 1, above + ties, 1.0 / ties), 32 KiB.  A thread
//   owns 4 cells (k, column) and adds to each in path order: every cell is ONE sequential f64 sum, then one division by
//   (double)S, so its bits depend on S and on that column's (above, ties) only.  A ragged last chunk runs a shorter loop
//   (the LDS rows past it are neither written nor read); columns >= G are staged as an empty block.  above / ties are
//   not validated: a ties <= 0 gives an empty block (the cell adds nothing), never an access outside the two matrices.
#pragma once

#include "bnf_totals.h"

namespace bnf {

constexpr int kRankMaxCols = BNF_RANK_MAX_COLS;     // the padded length at most
constexpr int kRankChunk = BNF_RANK_PATH_CHUNK;     // paths per LDS chunk of k_rank_probabilities
constexpr int kRankSlab = 64;                       // columns per workgroup of k_rank_probabilities
constexpr int kRankCells = 4;                       // cells (consecutive k) per thread
constexpr int kRankKPerBlock = (256 / kRankSlab) * kRankCells;
constexpr uint64_t kRankPad = ~0ull;
static_assert((kRankMaxCols & (kRankMaxCols - 1)) == 0, "the cap is a power of two: it is the padded length itself");
static_assert(sizeof(uint64_t) * kRankMaxCols <= 128 * 1024, "LDS per workgroup");
static_assert(kRankChunk % (256 / kRankSlab) == 0, "a staging pass is 4 paths of 64 columns");
static_assert((2 * sizeof(int32_t) + sizeof(double)) * kRankChunk * kRankSlab <= 40 * 1024, "four workgroups per CU");

// unsigned order of the keys == the total order of the values: NaN < -inf < ... < -0.0 == +0.0 < ... < +inf
__device__ __forceinline__ uint64_t rank_key(double v) {
  if (v != v) return 0ull;
  const uint64_t b = (uint64_t)__double_as_longlong(v == 0.0 ? 0.0 : v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ double rank_value(const double* __restrict__ row, const double* __restrict__ scale, int g) {
  return scale ? row[g] / scale[g] : row[g];
}

// blockDim.x a multiple of 64, at most 1,024.  P a power of two >= G, P <= kRankMaxCols; 8 P bytes of dynamic LDS.
__global__ __launch_bounds__(1024) void k_sample_ranks(const double* __restrict__ x, int64_t S, int32_t G, int32_t P,
                                                       const double* __restrict__ scale, double* __restrict__ out_rank,
                                                       int32_t* __restrict__ out_above, int32_t* __restrict__ out_ties) {
  extern __shared__ __attribute__((aligned(16))) uint64_t rank_sm[];
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int64_t s = blockIdx.x; s < S; s += gridDim.x) {
    const double* row = x + s * G;
    for (int i = tid; i < P; i += nt) rank_sm[i] = i < G ? rank_key(rank_value(row, scale, i)) : kRankPad;
    for (int k = 2; k <= P; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        __syncthreads();
        for (int i = tid; i < (P >> 1); i += nt) {
          const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1));
          const int hi = lo | j;
          const uint64_t u = rank_sm[lo], w = rank_sm[hi];
          if ((u > w) == ((lo & k) == 0)) { rank_sm[lo] = w; rank_sm[hi] = u; }
        }
      }
    }
    __syncthreads();
    // LDS holds the sorted keys only, so a column's own key is formed again from x and scale (the same loads and the same
    // IEEE division as at the fill: the same bits); keeping the unsorted keys as well would halve the columns that fit
    for (int g = tid; g < G; g += nt) {
      const uint64_t key = rank_key(rank_value(row, scale, g));
      int lo = 0, hi = G;                              // the first cell >= key
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (rank_sm[mid] < key) lo = mid + 1; else hi = mid;
      }
      const int lb = lo;
      hi = G;                                          // the first cell > key; it is past lb: the key itself is there
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (rank_sm[mid] <= key) lo = mid + 1; else hi = mid;
      }
      const int ties = lo - lb, above = G - lo;
      const int64_t o = s * G + g;
      if (out_above) out_above[o] = above;
      if (out_ties) out_ties[o] = ties;
      if (out_rank) out_rank[o] = (double)above + 0.5 * (double)(ties + 1);
    }
    __syncthreads();                                   // the next path overwrites the keys
  }
}

// grid (ceil(G / 64), ceil(K / 16)), 256 threads: thread (column lc, lane lr) owns k = 16 blockIdx.y + 4 lr + 1 .. + 4
__global__ __launch_bounds__(256) void k_rank_probabilities(const int32_t* __restrict__ above,
                                                            const int32_t* __restrict__ ties, int64_t S, int64_t G,
                                                            int32_t K, double* __restrict__ out) {
  __shared__ int32_t lo_[kRankChunk * kRankSlab];     // above + 1: the first rank slot of the block
  __shared__ int32_t hi_[kRankChunk * kRankSlab];     // above + ties: its last
  __shared__ double inv_[kRankChunk * kRankSlab];     // 1.0 / ties: the share of a slot
  const int tid = threadIdx.x, lc = tid & (kRankSlab - 1), lr = tid / kRankSlab;
  const int64_t c = (int64_t)blockIdx.x * kRankSlab + lc;
  const bool ok = c < G;
  const int32_t k0 = (int32_t)blockIdx.y * kRankKPerBlock + lr * kRankCells + 1;
  double acc[kRankCells];
#pragma unroll
  for (int i = 0; i < kRankCells; ++i) acc[i] = 0.0;

  for (int64_t s0 = 0; s0 < S; s0 += kRankChunk) {
    const int n = S - s0 < kRankChunk ? (int)(S - s0) : kRankChunk;
    __syncthreads();                                   // the previous chunk's reads are done
#pragma unroll
    for (int p = 0; p < kRankChunk / (256 / kRankSlab); ++p) {
      const int r = lr + (256 / kRankSlab) * p;
      if (r < n) {
        int32_t lo = 0x7fffffff, hi = 0;               // an empty block
        double inv = 0.0;
        if (ok) {
          const int64_t a = above[(s0 + r) * G + c], t = ties[(s0 + r) * G + c];
          const int64_t l = a + 1, h = a + t;          // formed in 64 bits: any int32 pair stays in range
          lo = (int32_t)(l > 0x7fffffffLL ? 0x7fffffffLL : l);
          hi = (int32_t)(h > 0x7fffffffLL ? 0x7fffffffLL : h < -0x7fffffffLL ? -0x7fffffffLL : h);
          inv = 1.0 / (double)t;
        }
        lo_[r * kRankSlab + lc] = lo;
        hi_[r * kRankSlab + lc] = hi;
        inv_[r * kRankSlab + lc] = inv;
      }
    }
    __syncthreads();
    for (int ss = 0; ss < n; ++ss) {
      const int32_t lo = lo_[ss * kRankSlab + lc], hi = hi_[ss * kRankSlab + lc];
      const double inv = inv_[ss * kRankSlab + lc];
#pragma unroll
      for (int i = 0; i < kRankCells; ++i)
        if (k0 + i >= lo && k0 + i <= hi) acc[i] = acc[i] + inv;
    }
  }
  if (ok) {
    const double dS = (double)S;
#pragma unroll
    for (int i = 0; i < kRankCells; ++i)
      if (k0 + i <= K) out[(int64_t)(k0 + i - 1) * G + c] = acc[i] / dS;
  }
}

}  // namespace bnf
