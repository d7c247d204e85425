// bnf_combinations.h -- linear combinations of the rows of the sample paths (bnf_predictive_combinations):
//   out[s][k] = sum over the positions p of form k of coef[p] * draw(s, rows[p]),   out (S, K) f64,
// without materialising the S x R draws.  Means and weighted means, contrasts and overlapping groups (a row in its county,
// its state and the nation) are all this object; the group totals of bnf_sampling.h are the case "every row once, every
// coefficient 1".
//
// The forms arrive as CSR over POSITIONS: form k owns the positions [form_offsets[k], form_offsets[k + 1]) of form_rows and
// form_coef.  A row may stand at any number of positions, of one form or of several, or at none: the draw is a pure
// function of (seed, path, global row), so every occurrence sees the same value, and a row at m positions is drawn m
// times (nothing is cached: a cache keyed by row would put an order on the blocks).
//
// The scheme is k_predictive_group_sums' (bnf_sampling.h) with the position count P in place of the row count on the
// position axis and one f64 multiply per position:
//   pass 1 (k_predictive_combinations, block = tile of kPredTile positions, strided over the samples): draws the tile's
//     values, widens them, multiplies each by its coefficient and sums every piece (form x tile) in f64 -- a one-piece
//     tile by the fixed tree (4 per thread, wave butterfly, 4 waves), a mixed tile by the segmented Hillis-Steele scan in
//     LDS.  A form inside the tile goes to out; a piece of a form that crosses a tile edge goes to the tile's slot 0 or 1
//     of partial (S, tiles, 2).
//   pass 2 (k_predictive_group_combine, unchanged, called with P for R): one wave per (first tile of a crossing form,
//     sample) adds that form's pieces in tile order.
// Same tiles, same trees, and x * 1.0 is exact: for a partition with unit coefficients the bits are those of
// bnf_predictive_group_sums.  The product is never contracted into the sum that follows it.
#pragma once

#include "bnf_sampling.h"

namespace bnf {

__device__ __forceinline__ double comb_term(double coef, float x) {
#pragma clang fp contract(off)
  return coef * (double)x;
}

// R: rows of loc (the table), P: positions of the CSR; grid.x = ceil(P / kPredTile)
template <int OBS>
__global__ __launch_bounds__(256) void k_predictive_combinations(
    const float* __restrict__ loc, const float* __restrict__ aux, int32_t M, int64_t R, int64_t P,
    const int32_t* __restrict__ form_offsets, const int32_t* __restrict__ form_rows,
    const double* __restrict__ form_coef, int32_t K, int64_t S, uint64_t seed, int64_t row0, int64_t sample0,
    const double* __restrict__ cum, double* __restrict__ partial, double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double xs[2][kPredTile];
  __shared__ double wsum[2][4];
  __shared__ int s_maxlen, s_kind, s_g;
  const int tid = threadIdx.x;
  const int64_t tile = blockIdx.x, n_tiles = gridDim.x;
  const int64_t tile0 = tile * kPredTile;
  const int64_t tile_end = tile0 + kPredTile < P ? tile0 + kPredTile : P;
  const int n_valid = (int)(tile_end - tile0);

  int32_t row[kPredRowsPerThread], ps[kPredRowsPerThread], grp[kPredRowsPerThread];
  int kind[kPredRowsPerThread];
  double cf[kPredRowsPerThread];
  if (tid == 0) s_maxlen = 0;
  __syncthreads();
  int maxlen = 0;
#pragma unroll
  for (int i = 0; i < kPredRowsPerThread; ++i) {
    const int q = i * 256 + tid;
    row[i] = -1; ps[i] = q; grp[i] = 0; kind[i] = PRED_DEST_NONE; cf[i] = 0.0;
    if (q < n_valid) {
      const int64_t p = tile0 + q;
      const int32_t g = pred_group_of(form_offsets, K, p);
      const int64_t o0 = form_offsets[g], o1 = form_offsets[g + 1];
      const int32_t rr = form_rows[p];
      row[i] = (rr >= 0 && (int64_t)rr < R) ? rr : -1;       // a row outside the table adds nothing
      cf[i] = form_coef[p];
      grp[i] = g;
      const int64_t rel = o0 - tile0;
      ps[i] = rel < 0 ? 0 : (rel > q ? q : (int)rel);
      maxlen = max(maxlen, q - ps[i] + 1);
      if (p + 1 == o1 || p + 1 == tile_end)
        kind[i] = (o0 >= tile0 && o1 <= tile_end) ? PRED_DEST_OUT : (o0 <= tile0 ? PRED_DEST_SLOT0 : PRED_DEST_SLOT1);
      if (p + 1 == tile_end) { s_kind = kind[i]; s_g = g; }
    }
  }
  atomicMax(&s_maxlen, maxlen);                              // integer, in LDS: order-free
  __syncthreads();
  const bool one_piece = s_maxlen == n_valid;                // block-uniform
  int n_steps = 0;
  while ((1 << n_steps) < s_maxlen) ++n_steps;
  const int u_kind = s_kind, u_g = s_g;

  int it = 0;
  for (int64_t s = blockIdx.y; s < S; s += gridDim.y, ++it) {
    const uint32_t sg = (uint32_t)(sample0 + s);
    const int32_t c = pred_component(seed, sg, M, cum);
    const float a0 = aux[c * 3], a1 = aux[c * 3 + 1], a2 = aux[c * 3 + 2];
    const float* lrow = loc + (int64_t)c * R;
    double v[kPredRowsPerThread];
#pragma unroll 1
    for (int i = 0; i < kPredRowsPerThread; ++i)
      v[i] = row[i] >= 0
                 ? comb_term(cf[i], predictive_draw<OBS>(seed, sg, (uint64_t)(row0 + row[i]), lrow[row[i]], a0, a1, a2))
                 : 0.0;
    if (one_piece) {
      const double t = wave_sum_f64(((v[0] + v[1]) + v[2]) + v[3]);
      if ((tid & 63) == 0) wsum[it & 1][tid >> 6] = t;
      __syncthreads();
      if (tid == 0)
        pred_store_piece(u_kind, u_g, ((wsum[it & 1][0] + wsum[it & 1][1]) + wsum[it & 1][2]) + wsum[it & 1][3], s, K, tile,
                         n_tiles, partial, out);
    } else {
      if (n_steps > 0) {
        __syncthreads();                                     // the previous sample's last step has read xs
#pragma unroll
        for (int i = 0; i < kPredRowsPerThread; ++i) xs[0][i * 256 + tid] = v[i];
        for (int k = 0; k < n_steps; ++k) {
          __syncthreads();
#pragma unroll
          for (int i = 0; i < kPredRowsPerThread; ++i) {
            const int q = i * 256 + tid, from = q - (1 << k);
            if (from >= ps[i]) v[i] += xs[k & 1][from];
            xs[(k + 1) & 1][q] = v[i];
          }
        }
      }
#pragma unroll
      for (int i = 0; i < kPredRowsPerThread; ++i) pred_store_piece(kind[i], grp[i], v[i], s, K, tile, n_tiles, partial, out);
    }
  }
}

}  // namespace bnf
