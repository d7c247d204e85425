// bnf_extremes.h -- group peaks and threshold exceedances of the posterior-predictive sample paths
// (bnf_predictive_group_extremes): per (path s, group g) the largest draw over the group's rows, the table row at which it
// is first reached and the number of rows whose draw exceeds that row's threshold, without materialising the S x R draws.
// The sibling of k_predictive_group_sums / k_predictive_group_combine (bnf_sampling.h) with another reduction: the same
// draws (predictive_draw<OBS>, pred_component: the floats bnf_predictive_samples would store, bit for bit), the same CSR
// input, the same tiling of the POSITION axis into kPredTile = 1024 and the same launch shape.
//
// The reduction runs on pieces (v, pos, cnt): v the f32 draw, pos its CSR position, cnt an integer count.
//   b beats a  iff  b.v > a.v, or b.v == a.v and b.pos < a.pos;   the counts add.
// A NaN draw enters as v = -inf (with its position) and never exceeds a threshold, so the operator is a total order on
// (v descending, pos ascending): associative and commutative.  The result cannot depend on tile edges, the launch
// geometry or how the samples are cut into passes; positions ascend with the table row inside a group (csr_from_codes
// sorts stably), so a tie goes to the lowest table row.  An entry of seg_rows outside [0, R) is the identity
// (-inf, kExtNoPos, 0): it takes no part.  A group without a row that takes part reports max NaN, argmax -1, count 0.
//   pass 1 (k_predictive_group_extremes, block = tile, strided over the samples): a tile inside one group reduces by a
//     fixed tree (4 per thread, wave butterfly, 4 waves); a mixed tile by a segmented Hillis-Steele scan in LDS.  A group
//     inside the tile is finished here; a piece of a group that crosses a tile edge goes to the tile's slot 0 (the group
//     holds the tile's first position) or slot 1 (partial: (S, tiles, 2) ExtPiece).
//   pass 2 (k_predictive_group_extremes_combine): one wave per (first tile of a crossing group, sample) joins that
//     group's pieces in tile order.
// No floating-point atomics.  The two per-row counters are integer atomicAdd only (order-free): exceed_count[r] once per
// thread and row after the thread's samples, peak_count[r] once per finished (path, group).
#pragma once

#include "bnf_sampling.h"

namespace bnf {

constexpr int32_t kExtNoPos = 0x7fffffff;      // no CSR position is this large: R <= 2^31 - 1

struct ExtPiece {
  float v;
  int32_t pos;
  int32_t cnt;
  int32_t pad;
};
static_assert(sizeof(ExtPiece) * 2 == BNF_EXTREMES_WORK_PER_TILE, "work buffer: two pieces per tile and path");

__device__ __forceinline__ void ext_join(float& v, int32_t& pos, float bv, int32_t bpos) {
  if (bv > v || (bv == v && bpos < pos)) { v = bv; pos = bpos; }
}

__device__ __forceinline__ void ext_wave_join(float& v, int32_t& pos, int32_t& cnt) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float bv = __shfl_xor(v, off, 64);
    const int32_t bpos = __shfl_xor(pos, off, 64);
    cnt += __shfl_xor(cnt, off, 64);
    ext_join(v, pos, bv, bpos);
  }
}

struct ExtOut {
  const int32_t* seg_rows;
  double* max;           // (S, G)
  int32_t* argmax;       // (S, G) or null
  double* count;         // (S, G) or null
  uint32_t* peak_count;  // (R,) or null
};

// the finished piece of (path s, group g)
__device__ __forceinline__ void ext_store_final(const ExtOut& o, int64_t s, int32_t g, int32_t G, float v, int32_t pos,
                                                int32_t cnt) {
  const int64_t idx = s * G + g;
  const bool none = pos == kExtNoPos;
  const int32_t row = none ? -1 : o.seg_rows[pos];
  o.max[idx] = none ? __builtin_nan("") : (double)v;
  if (o.argmax) o.argmax[idx] = row;
  if (o.count) o.count[idx] = (double)cnt;
  if (o.peak_count && row >= 0) atomicAdd(&o.peak_count[row], 1u);
}

__device__ __forceinline__ void ext_store_piece(int kind, int32_t g, float v, int32_t pos, int32_t cnt, int64_t s, int32_t G,
                                                int64_t tile, int64_t n_tiles, ExtPiece* __restrict__ partial,
                                                const ExtOut& o) {
  if (kind == PRED_DEST_OUT) ext_store_final(o, s, g, G, v, pos, cnt);
  else if (kind != PRED_DEST_NONE) partial[(s * n_tiles + tile) * 2 + (kind - PRED_DEST_SLOT0)] = ExtPiece{v, pos, cnt, 0};
}

template <int OBS>
__global__ __launch_bounds__(256) void k_predictive_group_extremes(
    const float* __restrict__ loc, const float* __restrict__ aux, int32_t M, int64_t R,
    const int32_t* __restrict__ seg_offsets, const int32_t* __restrict__ seg_rows, int32_t G, int64_t S, uint64_t seed,
    int64_t row0, int64_t sample0, const double* __restrict__ cum, const float* __restrict__ threshold,
    ExtPiece* __restrict__ partial, ExtOut o, uint32_t* __restrict__ exceed_count) {
  __shared__ float xv[2][kPredTile];
  __shared__ int32_t xp[2][kPredTile];
  __shared__ int32_t xc[2][kPredTile];
  __shared__ float wv[2][4];
  __shared__ int32_t wp[2][4], wc[2][4];
  __shared__ int s_maxlen, s_kind, s_g;
  const int tid = threadIdx.x;
  const int64_t tile = blockIdx.x, n_tiles = gridDim.x;
  const int64_t tile0 = tile * kPredTile;
  const int64_t tile_end = tile0 + kPredTile < R ? tile0 + kPredTile : R;
  const int n_valid = (int)(tile_end - tile0);

  int32_t row[kPredRowsPerThread], ps[kPredRowsPerThread], grp[kPredRowsPerThread];
  int kind[kPredRowsPerThread];
  float thr[kPredRowsPerThread];
  uint32_t exc[kPredRowsPerThread];
  if (tid == 0) s_maxlen = 0;
  __syncthreads();
  int maxlen = 0;
#pragma unroll
  for (int i = 0; i < kPredRowsPerThread; ++i) {
    const int q = i * 256 + tid;
    row[i] = -1; ps[i] = q; grp[i] = 0; kind[i] = PRED_DEST_NONE; thr[i] = 0.f; exc[i] = 0u;
    if (q < n_valid) {
      const int64_t p = tile0 + q;
      const int32_t g = pred_group_of(seg_offsets, G, p);
      const int64_t o0 = seg_offsets[g], o1 = seg_offsets[g + 1];
      const int32_t rr = seg_rows[p];
      row[i] = (rr >= 0 && (int64_t)rr < R) ? rr : -1;       // a row outside the table takes no part
      if (threshold && row[i] >= 0) thr[i] = threshold[row[i]];
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
    float v[kPredRowsPerThread];
    int32_t pos[kPredRowsPerThread], cnt[kPredRowsPerThread];
#pragma unroll 1
    for (int i = 0; i < kPredRowsPerThread; ++i) {
      v[i] = -INFINITY; pos[i] = kExtNoPos; cnt[i] = 0;
      if (row[i] >= 0) {
        const float x = predictive_draw<OBS>(seed, sg, (uint64_t)(row0 + row[i]), lrow[row[i]], a0, a1, a2);
        if (threshold && x > thr[i]) { cnt[i] = 1; ++exc[i]; }      // false for a NaN draw
        v[i] = x != x ? -INFINITY : x;
        pos[i] = (int32_t)(tile0 + i * 256 + tid);
      }
    }
    if (one_piece) {
      float tv = v[0];
      int32_t tp = pos[0], tc = ((cnt[0] + cnt[1]) + cnt[2]) + cnt[3];
#pragma unroll
      for (int i = 1; i < kPredRowsPerThread; ++i) ext_join(tv, tp, v[i], pos[i]);
      ext_wave_join(tv, tp, tc);
      if ((tid & 63) == 0) { wv[it & 1][tid >> 6] = tv; wp[it & 1][tid >> 6] = tp; wc[it & 1][tid >> 6] = tc; }
      __syncthreads();
      if (tid == 0) {
        tv = wv[it & 1][0]; tp = wp[it & 1][0]; tc = wc[it & 1][0];
#pragma unroll
        for (int w = 1; w < 4; ++w) { ext_join(tv, tp, wv[it & 1][w], wp[it & 1][w]); tc += wc[it & 1][w]; }
        ext_store_piece(u_kind, u_g, tv, tp, tc, s, G, tile, n_tiles, partial, o);
      }
    } else {
      if (n_steps > 0) {
        __syncthreads();                                     // the previous sample's last step has read the buffers
#pragma unroll
        for (int i = 0; i < kPredRowsPerThread; ++i) {
          const int q = i * 256 + tid;
          xv[0][q] = v[i]; xp[0][q] = pos[i]; xc[0][q] = cnt[i];
        }
        for (int k = 0; k < n_steps; ++k) {
          __syncthreads();
#pragma unroll
          for (int i = 0; i < kPredRowsPerThread; ++i) {
            const int q = i * 256 + tid, from = q - (1 << k);
            if (from >= ps[i]) {
              ext_join(v[i], pos[i], xv[k & 1][from], xp[k & 1][from]);
              cnt[i] += xc[k & 1][from];
            }
            xv[(k + 1) & 1][q] = v[i]; xp[(k + 1) & 1][q] = pos[i]; xc[(k + 1) & 1][q] = cnt[i];
          }
        }
      }
#pragma unroll
      for (int i = 0; i < kPredRowsPerThread; ++i)
        ext_store_piece(kind[i], grp[i], v[i], pos[i], cnt[i], s, G, tile, n_tiles, partial, o);
    }
  }
  if (exceed_count) {
#pragma unroll
    for (int i = 0; i < kPredRowsPerThread; ++i)
      if (exc[i]) atomicAdd(&exceed_count[row[i]], exc[i]);      // exc > 0 only where row >= 0
  }
}

// pass 2: block = 4 waves, wave = (tile blockIdx.x, sample blockIdx.y * 4 + wave).  Only the wave of a tile in which a
// group STARTS and which that group leaves through the far edge has work: it owns that group's result.
__global__ __launch_bounds__(256) void k_predictive_group_extremes_combine(const int32_t* __restrict__ seg_offsets,
                                                                           int32_t G, int64_t R, int64_t S,
                                                                           const ExtPiece* __restrict__ partial, ExtOut o) {
  const int64_t s = (int64_t)blockIdx.y * 4 + (threadIdx.x >> 6);
  if (s >= S) return;
  const int lane = threadIdx.x & 63;
  const int64_t tile = blockIdx.x, n_tiles = gridDim.x;
  const int64_t tile0 = tile * kPredTile;
  const int64_t tile_end = tile0 + kPredTile < R ? tile0 + kPredTile : R;
  const int32_t g = pred_group_of(seg_offsets, G, tile_end - 1);
  const int64_t o0 = seg_offsets[g], o1 = seg_offsets[g + 1];
  if (o0 < tile0 || o1 <= tile_end) return;
  const int64_t last = (o1 - 1) / kPredTile;
  float v = -INFINITY;
  int32_t pos = kExtNoPos, cnt = 0;
  for (int64_t j = tile + lane; j <= last && j < n_tiles; j += 64) {
    const ExtPiece b = partial[(s * n_tiles + j) * 2 + ((j == tile && o0 != tile0) ? 1 : 0)];
    ext_join(v, pos, b.v, b.pos);
    cnt += b.cnt;
  }
  ext_wave_join(v, pos, cnt);
  if (lane == 0) ext_store_final(o, s, g, G, v, pos, cnt);
}

}  // namespace bnf
