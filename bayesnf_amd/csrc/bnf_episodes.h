// bnf_episodes.h -- spells above a threshold in the posterior-predictive sample paths (bnf_predictive_group_episodes):
// per (path s, group g) the longest run of consecutive positions whose draw exceeds its row's threshold and the table
// row at which it starts, the number of maximal runs, the number of steps before the first exceedance and the table rows
// of the first and last exceedance, without materialising the S x R draws.  The sibling of k_predictive_group_extremes
// (bnf_extremes.h): the same draws (predictive_draw<OBS>, pred_component: the floats bnf_predictive_samples would store,
// bit for bit), the same CSR input, the same tiling of the POSITION axis into kPredTile = 1024, the same launch shape and
// the same two passes over a work buffer.  TIME is the order of the positions inside a group.
//
// The reduction runs on pieces (EpPiece) that describe a contiguous stretch of participating positions:
//   len        participating positions
//   lead       non-exceeding positions before the first exceeding one (= len when none exceeds)
//   pre        length of the leading run            suf, suf_pos   length and first position of the trailing run
//   best, best_pos   the longest run and its first position (the earliest among equally long ones)
//   runs       maximal runs            first, last   first and last exceeding position
// ep_join(a, b), a BEFORE b, is associative and all-integer, so the result cannot depend on tile edges, the launch
// geometry or how the samples are cut into passes.  It is NOT commutative: every step below keeps position order (the
// xor butterfly and the lane-strided combine of the extremes would not).  A NaN draw does not exceed but takes part (it
// breaks a run and counts as a step); an entry of seg_rows outside [0, R) is the identity (all zero, no position).
//   pass 1 (k_predictive_group_episodes, block = tile, strided over the samples): thread t owns the 4 CONSECUTIVE
//     positions 4t .. 4t + 3 and folds them one by one (ep_push).  Its piece since the last group start inside it, with a
//     flag "a group starts here", goes through a segmented shift-up scan over the 256 threads (6 __shfl_up steps inside
//     a wave, the 4 wave totals through LDS, joined in wave order); the exclusive result is what the group that reaches
//     into the thread has gathered before it.  The thread folds its positions once more on top of that and stores at every
//     position that ends a group or the tile: a group inside the tile is finished here; a piece of a group that crosses
//     a tile edge goes to the tile's slot 0 (the group holds the tile's first position) or slot 1
//     (partial: (S, tiles, 2) EpPiece).  One path for tiles inside one group and for mixed tiles.
//   pass 2 (k_predictive_group_episodes_combine): one wave per (first tile of a crossing group, sample).  Lane l joins a
//     CONTIGUOUS range of that group's tiles in tile order, then a shift-down tree joins the 64 lanes in lane order.
// LDS: 2 x 4 wave totals of 11 words = 352 bytes (the pieces never go through LDS one per position).
// No floating-point atomics.  onset_count[r] is integer atomicAdd only (order-free), once per finished (path, group).
#pragma once

#include "bnf_sampling.h"

namespace bnf {

constexpr int32_t kEpNoPos = -1;

struct EpPiece {
  int32_t len, lead, pre, suf, suf_pos, best, best_pos, runs, first, last;
};
static_assert(sizeof(EpPiece) * 2 == BNF_EPISODES_WORK_PER_TILE, "work buffer: two pieces per tile and path");

__device__ __forceinline__ EpPiece ep_identity() { return EpPiece{0, 0, 0, 0, kEpNoPos, 0, kEpNoPos, 0, kEpNoPos, kEpNoPos}; }

// a followed by one participating position
__device__ __forceinline__ void ep_push(EpPiece& a, bool exceeds, int32_t pos) {
  if (exceeds) {
    if (a.suf == 0) { a.suf_pos = pos; ++a.runs; }
    ++a.suf;
    if (a.pre == a.len) ++a.pre;
    if (a.first < 0) a.first = pos;
    a.last = pos;
    if (a.suf > a.best) { a.best = a.suf; a.best_pos = a.suf_pos; }
  } else {
    a.suf = 0; a.suf_pos = kEpNoPos;
    if (a.best == 0) ++a.lead;
  }
  ++a.len;
}

// a BEFORE b
__device__ __forceinline__ EpPiece ep_join(const EpPiece& a, const EpPiece& b) {
  EpPiece r;
  r.len = a.len + b.len;
  r.lead = a.best == 0 ? a.len + b.lead : a.lead;
  r.pre = a.pre == a.len ? a.len + b.pre : a.pre;
  const bool b_all = b.suf == b.len;
  r.suf = b_all ? b.len + a.suf : b.suf;
  r.suf_pos = (b_all && a.suf > 0) ? a.suf_pos : b.suf_pos;
  const int32_t mid = a.suf + b.pre, mid_pos = a.suf > 0 ? a.suf_pos : b.first;
  r.best = a.best; r.best_pos = a.best_pos;
  if (mid > r.best) { r.best = mid; r.best_pos = mid_pos; }          // strict >: the earliest run wins a tie
  if (b.best > r.best) { r.best = b.best; r.best_pos = b.best_pos; }
  r.runs = a.runs + b.runs - ((a.suf > 0 && b.pre > 0) ? 1 : 0);
  r.first = a.first >= 0 ? a.first : b.first;
  r.last = b.last >= 0 ? b.last : a.last;
  return r;
}

__device__ __forceinline__ EpPiece ep_shfl_up(const EpPiece& a, int off) {
  return EpPiece{__shfl_up(a.len, off, 64), __shfl_up(a.lead, off, 64), __shfl_up(a.pre, off, 64), __shfl_up(a.suf, off, 64),
                 __shfl_up(a.suf_pos, off, 64), __shfl_up(a.best, off, 64), __shfl_up(a.best_pos, off, 64),
                 __shfl_up(a.runs, off, 64), __shfl_up(a.first, off, 64), __shfl_up(a.last, off, 64)};
}

__device__ __forceinline__ EpPiece ep_shfl_down(const EpPiece& a, int off) {
  return EpPiece{__shfl_down(a.len, off, 64), __shfl_down(a.lead, off, 64), __shfl_down(a.pre, off, 64),
                 __shfl_down(a.suf, off, 64), __shfl_down(a.suf_pos, off, 64), __shfl_down(a.best, off, 64),
                 __shfl_down(a.best_pos, off, 64), __shfl_down(a.runs, off, 64), __shfl_down(a.first, off, 64),
                 __shfl_down(a.last, off, 64)};
}

struct EpOut {
  const int32_t* seg_rows;
  double* longest;          // (S, G)
  int32_t* longest_row;     // (S, G) or null
  double* spells;           // (S, G) or null
  double* onset_step;       // (S, G) or null
  int32_t* first_row;       // (S, G) or null
  int32_t* last_row;        // (S, G) or null
  uint32_t* onset_count;    // (R,) or null
};

// the finished piece of (path s, group g); a position a piece carries is one that took part: its row lies in [0, R)
__device__ __forceinline__ void ep_store_final(const EpOut& o, int64_t s, int32_t g, int32_t G, const EpPiece& a) {
  const int64_t idx = s * G + g;
  o.longest[idx] = (double)a.best;
  if (o.longest_row) o.longest_row[idx] = a.best > 0 ? o.seg_rows[a.best_pos] : -1;
  if (o.spells) o.spells[idx] = (double)a.runs;
  if (o.onset_step) o.onset_step[idx] = (double)a.lead;
  const int32_t row = a.first >= 0 ? o.seg_rows[a.first] : -1;
  if (o.first_row) o.first_row[idx] = row;
  if (o.last_row) o.last_row[idx] = a.last >= 0 ? o.seg_rows[a.last] : -1;
  if (o.onset_count && row >= 0) atomicAdd(&o.onset_count[row], 1u);
}

__device__ __forceinline__ void ep_store_piece(int kind, int32_t g, const EpPiece& a, int64_t s, int32_t G, int64_t tile,
                                               int64_t n_tiles, EpPiece* __restrict__ partial, const EpOut& o) {
  if (kind == PRED_DEST_OUT) ep_store_final(o, s, g, G, a);
  else if (kind != PRED_DEST_NONE) partial[(s * n_tiles + tile) * 2 + (kind - PRED_DEST_SLOT0)] = a;
}

template <int OBS>
__global__ __launch_bounds__(256) void k_predictive_group_episodes(
    const float* __restrict__ loc, const float* __restrict__ aux, int32_t M, int64_t R,
    const int32_t* __restrict__ seg_offsets, const int32_t* __restrict__ seg_rows, int32_t G, int64_t S, uint64_t seed,
    int64_t row0, int64_t sample0, const double* __restrict__ cum, const float* __restrict__ threshold,
    EpPiece* __restrict__ partial, EpOut o) {
  __shared__ EpPiece wpiece[2][4];
  __shared__ int32_t wflag[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t tile = blockIdx.x, n_tiles = gridDim.x;
  const int64_t tile0 = tile * kPredTile;
  const int64_t tile_end = tile0 + kPredTile < R ? tile0 + kPredTile : R;
  const int n_valid = (int)(tile_end - tile0);

  // thread t owns the consecutive positions 4 t .. 4 t + 3 of the tile
  int32_t row[kPredRowsPerThread], grp[kPredRowsPerThread];
  int kind[kPredRowsPerThread];
  bool start[kPredRowsPerThread];
  float thr[kPredRowsPerThread];
  bool any_start = false;
#pragma unroll
  for (int i = 0; i < kPredRowsPerThread; ++i) {
    const int q = tid * kPredRowsPerThread + i;
    row[i] = -1; grp[i] = 0; kind[i] = PRED_DEST_NONE; start[i] = false; thr[i] = 0.f;
    if (q < n_valid) {
      const int64_t p = tile0 + q;
      const int32_t g = pred_group_of(seg_offsets, G, p);
      const int64_t o0 = seg_offsets[g], o1 = seg_offsets[g + 1];
      const int32_t rr = seg_rows[p];
      row[i] = (rr >= 0 && (int64_t)rr < R) ? rr : -1;       // a row outside the table takes no part
      if (row[i] >= 0) thr[i] = threshold[row[i]];
      grp[i] = g;
      start[i] = p == o0 || q == 0;
      any_start = any_start || start[i];
      if (p + 1 == o1 || p + 1 == tile_end)
        kind[i] = (o0 >= tile0 && o1 <= tile_end) ? PRED_DEST_OUT : (o0 <= tile0 ? PRED_DEST_SLOT0 : PRED_DEST_SLOT1);
    }
  }

  int it = 0;
  for (int64_t s = blockIdx.y; s < S; s += gridDim.y, ++it) {
    const uint32_t sg = (uint32_t)(sample0 + s);
    const int32_t c = pred_component(seed, sg, M, cum);
    const float a0 = aux[c * 3], a1 = aux[c * 3 + 1], a2 = aux[c * 3 + 2];
    const float* lrow = loc + (int64_t)c * R;
    uint32_t exc = 0u;                                         // bit i: position 4 t + i exceeds
#pragma unroll 1
    for (int i = 0; i < kPredRowsPerThread; ++i) {
      if (row[i] >= 0) {
        const float x = predictive_draw<OBS>(seed, sg, (uint64_t)(row0 + row[i]), lrow[row[i]], a0, a1, a2);
        if (x > thr[i]) exc |= 1u << i;                          // false for a NaN draw
      }
    }
    // the thread's piece since the last group start inside it
    EpPiece a = ep_identity();
#pragma unroll
    for (int i = 0; i < kPredRowsPerThread; ++i) {
      if (start[i]) a = ep_identity();
      if (row[i] >= 0) ep_push(a, (exc >> i) & 1u, (int32_t)(tile0 + tid * kPredRowsPerThread + i));
    }
    // segmented inclusive scan over the wave, earlier lanes on the left
    bool f = any_start;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const EpPiece b = ep_shfl_up(a, off);
      const int bf = __shfl_up((int)f, off, 64);
      if (lane >= off) {
        if (!f) a = ep_join(b, a);
        f = f || bf != 0;
      }
    }
    if (lane == 63) { wpiece[it & 1][wave] = a; wflag[it & 1][wave] = (int32_t)f; }
    __syncthreads();
    // what the group that reaches into this thread has gathered before it: the waves before this one in wave order,
    // then the lanes before this one
    EpPiece carry = ep_identity();
    for (int w = 0; w < wave; ++w) {
      const EpPiece b = wpiece[it & 1][w];
      carry = wflag[it & 1][w] ? b : ep_join(carry, b);
    }
    EpPiece cur = ep_shfl_up(a, 1);
    const int curf = __shfl_up((int)f, 1, 64);
    if (lane == 0) cur = carry;
    else if (!curf) cur = ep_join(carry, cur);
#pragma unroll
    for (int i = 0; i < kPredRowsPerThread; ++i) {
      if (start[i]) cur = ep_identity();
      if (row[i] >= 0) ep_push(cur, (exc >> i) & 1u, (int32_t)(tile0 + tid * kPredRowsPerThread + i));
      ep_store_piece(kind[i], grp[i], cur, s, G, tile, n_tiles, partial, o);
    }
  }
}

// pass 2: block = 4 waves, wave = (tile blockIdx.x, sample blockIdx.y * 4 + wave).  Only the wave of a tile in which a
// group STARTS and which that group leaves through the far edge has work: it owns that group's result.
__global__ __launch_bounds__(256) void k_predictive_group_episodes_combine(const int32_t* __restrict__ seg_offsets,
                                                                           int32_t G, int64_t R, int64_t S,
                                                                           const EpPiece* __restrict__ partial, EpOut o) {
  const int64_t s = (int64_t)blockIdx.y * 4 + (threadIdx.x >> 6);
  if (s >= S) return;
  const int lane = threadIdx.x & 63;
  const int64_t tile = blockIdx.x, n_tiles = gridDim.x;
  const int64_t tile0 = tile * kPredTile;
  const int64_t tile_end = tile0 + kPredTile < R ? tile0 + kPredTile : R;
  const int32_t g = pred_group_of(seg_offsets, G, tile_end - 1);
  const int64_t o0 = seg_offsets[g], o1 = seg_offsets[g + 1];
  if (o0 < tile0 || o1 <= tile_end) return;
  int64_t last = (o1 - 1) / kPredTile;
  if (last > n_tiles - 1) last = n_tiles - 1;
  const int64_t per = (last - tile + 1 + 63) / 64;           // lane l: the tiles tile + l per .. tile + (l + 1) per - 1
  const int64_t j0 = tile + lane * per;
  const int64_t j1 = j0 + per < last + 1 ? j0 + per : last + 1;
  EpPiece a = ep_identity();
  for (int64_t j = j0; j < j1; ++j)
    a = ep_join(a, partial[(s * n_tiles + j) * 2 + ((j == tile && o0 != tile0) ? 1 : 0)]);
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {                   // ordered tree: lane l takes lane l + off on its right
    const EpPiece b = ep_shfl_down(a, off);
    if ((lane & (2 * off - 1)) == 0) a = ep_join(a, b);
  }
  if (lane == 0) ep_store_final(o, s, g, G, a);
}

}  // namespace bnf
