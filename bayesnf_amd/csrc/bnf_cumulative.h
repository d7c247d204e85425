// bnf_cumulative.h -- running totals of the posterior-predictive sample paths (bnf_predictive_group_cumulative): per
// (path s, group g) the cumulative curve run[s][p] = the f64 sum of the draws at the participating positions of g up to
// and including p, its last value (the group total) and, against a per-group level, the first position at which the
// curve lies above it, without materialising the S x R draws.  A sibling of k_predictive_group_episodes (bnf_episodes.h):
// the same draws (predictive_draw<OBS>, pred_component: the floats bnf_predictive_samples would store, bit for bit,
// widened to f64), the same CSR input, the same tiling of the POSITION axis into kPredTile = 1024 and the same mapping
// thread t -> the 4 CONSECUTIVE positions 4t .. 4t + 3.  TIME is the order of the positions inside a group.
//
// An entry of seg_rows outside [0, R) takes no part: its run is the value carried so far (0 at a group's start) and it is
// not a step.  A NaN draw takes part: every later run of its group is NaN, it counts as a step, and `run > level` is
// false for it.
//
// ONE kernel, no work buffer, no combine pass, and no workgroup ever waits for another:
//   * block = tile (blockIdx.x), strided over the samples (blockIdx.y).  A block OWNS the groups that START in its tile.
//     The leading positions of a tile that belong to a group begun in an earlier tile are skipped (not drawn); a block
//     that owns nothing exits after one bisection.
//   * per path: every thread draws and folds its 4 positions; a segmented __shfl_up scan of (f64 sum, steps, "a group
//     starts here") runs over the wave, the 4 wave totals go through LDS and are joined in wave order; the exclusive
//     result is what the group that reaches into the thread has gathered before it.  The thread folds its positions once
//     more on top of that: the run at every position, stored to `running`, compared with the level, stored to `total`
//     at a group's last position.  With a level, a second segmented scan of an int32 with min (the first position above
//     the level since the group's start) tells every thread whether its group has crossed before it: the thread that
//     holds the first crossing position writes cross_step / cross_row and adds to cross_count; the thread at the group's
//     last position writes the censored values when the path never crossed.
//   * a group that leaves its tile through the far edge is FINISHED BY THE BLOCK OF THE TILE IT STARTS IN: that block
//     walks on over the following tiles, restricted to that group's positions, and carries (sum, steps so far, crossing
//     found) block-uniformly in LDS from one tile to the next.  Every position is drawn exactly once.  The group's last
//     piece, of fewer than 1024 positions, is spread over the threads (ceil(left / 256) consecutive positions each): the
//     few positions by which a short group reaches into the next tile then cost one draw of one wave, not four.
// The price: a long group is parallel over the sample axis only (the launch sizes grid.y for that, bnf_forecast.hip cum_grid).
//
// Order of the f64 additions (it follows the tiling, so it may depend on where a group lies on the position axis, and
// on nothing else): inside a thread left to right; lanes by the shift-up scan (left operand = the earlier lanes); waves
// in wave order; the carry of the earlier tiles is the left operand of the tile's prefix.  NB / ZINB: every sum is an
// exact integer below 2^53, the order plays no part.
// LDS: what the block knows of its own tile's positions (row, group, level, flags: 17 bytes per position, written once,
// read back by the thread that wrote it: registers are what bounds the occupancy of the NB draw) = 17,408 bytes, plus
// 2 x (4 wave totals of (f64, 3 x int32) + the carry (f64, 2 x int32)) = 192 bytes, double-buffered by the parity of a
// block-uniform chunk counter so that one barrier per scan suffices.
// No floating-point atomics.  cross_count[r], above_count[r] are integer atomicAdd only (order-free).
#pragma once

#include "bnf_sampling.h"

namespace bnf {

constexpr int32_t kCumNoPos = 0x7fffffff;

struct CumOut {
  const double* level;      // (G,) or null
  double* total;            // (S, G)
  double* running;          // (S, R) by position, or null
  double* cross_step;       // (S, G) or null
  int32_t* cross_row;       // (S, G) or null
  uint32_t* cross_count;    // (R,) or null
  uint32_t* above_count;    // (R,) or null
};

struct CumShared {
  double lvl[kPredTile];    // the home tile: level of the position's group
  int32_t row[kPredTile];   //   table row, -1: takes no part or is not this block's
  int32_t grp[kPredTile];   //   group
  uint32_t flags[256];      //   per thread, CUM_* << i for its position i
  double wsum[2][4];        // wave totals since the last group start in the wave
  double csum[2];           // carry of a group that walks on: its run at the end of the chunk before
  int32_t wsteps[2][4], wflag[2][4], wmin[2][4];
  int32_t csteps[2], cmin[2];
};

// per position i of a thread: a group starts here / ends here / the position is this block's (its run is stored)
enum : uint32_t { CUM_START = 1u, CUM_END = 1u << 4, CUM_STORED = 1u << 8 };

template <int OBS>
__global__ __launch_bounds__(256) void k_predictive_group_cumulative(
    const float* __restrict__ loc, const float* __restrict__ aux, int32_t M, int64_t R,
    const int32_t* __restrict__ seg_offsets, const int32_t* __restrict__ seg_rows, int32_t G, int64_t S, uint64_t seed,
    int64_t row0, int64_t sample0, const double* __restrict__ cum, CumOut o) {
  __shared__ __attribute__((aligned(16))) CumShared sh;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t tile0 = (int64_t)blockIdx.x * kPredTile;
  const int64_t tile_end = tile0 + kPredTile < R ? tile0 + kPredTile : R;
  const int n_valid = (int)(tile_end - tile0);
  const bool has_level = o.level != nullptr;

  // the block owns the positions from the first group start of its tile on; none: nothing to do (block-uniform)
  {
    const int32_t gf = pred_group_of(seg_offsets, G, tile0);
    const int64_t own0 = (int64_t)seg_offsets[gf] == tile0 ? tile0 : (int64_t)seg_offsets[gf + 1];
    if (own0 >= tile_end) return;
  }

  // thread t owns the consecutive positions 4 t .. 4 t + 3 of the tile; what it finds out about them is kept in LDS and
  // read back by itself alone (no barrier)
  {
    uint32_t flags = 0u;
#pragma unroll
    for (int i = 0; i < kPredRowsPerThread; ++i) {
      const int q = tid * kPredRowsPerThread + i;
      int32_t row = -1, grp = 0;
      double lvl = 0.0;
      if (q < n_valid) {
        const int64_t p = tile0 + q;
        const int32_t g = pred_group_of(seg_offsets, G, p);
        const int64_t o0 = seg_offsets[g], o1 = seg_offsets[g + 1];
        if (o0 >= tile0) {                                       // a group begun in an earlier tile is that tile's
          const int32_t rr = seg_rows[p];
          row = (rr >= 0 && (int64_t)rr < R) ? rr : -1;          // a row outside the table takes no part
          grp = g;
          if (has_level) lvl = o.level[g];
          flags |= CUM_STORED << i;
          if (p == o0) flags |= CUM_START << i;
          if (p + 1 == o1) flags |= CUM_END << i;
        }
      }
      sh.row[q] = row; sh.grp[q] = grp; sh.lvl[q] = lvl;
    }
    sh.flags[tid] = flags;
  }
  // the group that holds the tile's last position: if it starts here and goes on, this block walks on to its end
  const int32_t gw = pred_group_of(seg_offsets, G, tile_end - 1);
  int64_t wend = seg_offsets[gw + 1];
  if (wend > R) wend = R;
  const bool walk = (int64_t)seg_offsets[gw] >= tile0 && wend > tile_end;           // block-uniform
  const double wlevel = (walk && has_level) ? o.level[gw] : 0.0;

  int k = 0;                                                     // chunks done: its parity is the LDS buffer
  for (int64_t s = blockIdx.y; s < S; s += gridDim.y) {
    const uint32_t sg = (uint32_t)(sample0 + s);
    const int32_t c = pred_component(seed, sg, M, cum);
    const float a0 = aux[c * 3], a1 = aux[c * 3 + 1], a2 = aux[c * 3 + 2];
    const float* lrow = loc + (int64_t)c * R;
    // chunk = the home tile, then (walk) the tiles after it up to the end of the group that walks on
    int64_t base = tile0;
    for (bool home = true;; home = false) {
      const int b = k & 1;
      ++k;
      int32_t row[kPredRowsPerThread];
      uint32_t flags = 0u;
      int per = kPredRowsPerThread;                             // the thread owns the positions base + per tid + i, i < per
      if (home) {
        const int4 r4 = reinterpret_cast<const int4*>(sh.row)[tid];
        row[0] = r4.x; row[1] = r4.y; row[2] = r4.z; row[3] = r4.w;
        flags = sh.flags[tid];
      } else {
        // the group's last piece: its positions spread over the threads, 1 to 4 consecutive ones each -- the few
        // positions by which a short group reaches into the next tile cost one draw of one wave, not four
        if (wend - base < kPredTile) per = (int)((wend - base + 255) >> 8);
#pragma unroll
        for (int i = 0; i < kPredRowsPerThread; ++i) {
          const int64_t p = base + tid * per + i;
          row[i] = -1;
          if (i < per && p < wend) {
            const int32_t rr = seg_rows[p];
            row[i] = (rr >= 0 && (int64_t)rr < R) ? rr : -1;
            flags |= CUM_STORED << i;
            if (p + 1 == wend) flags |= CUM_END << i;
          }
        }
      }
      // this thread holds the chunk's last position and its group walks on: it hands the carry to the next chunk
      const bool carry_to = walk && tid == 255 && base + kPredTile < wend;

      float x[kPredRowsPerThread];
#pragma unroll 1
      for (int i = 0; i < kPredRowsPerThread; ++i)
        x[i] = row[i] >= 0 ? predictive_draw<OBS>(seed, sg, (uint64_t)(row0 + row[i]), lrow[row[i]], a0, a1, a2) : 0.f;

      // the thread's sum and steps since the last group start inside it
      double a = 0.0;
      int32_t n = 0;
      const bool f0 = (flags & 0xfu) != 0u;
#pragma unroll
      for (int i = 0; i < kPredRowsPerThread; ++i) {
        if (flags & (CUM_START << i)) { a = 0.0; n = 0; }
        if (row[i] >= 0) { a += (double)x[i]; ++n; }
      }
      // segmented inclusive scan over the wave, earlier lanes on the left
      bool f = f0;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const double ba = __shfl_up(a, off, 64);
        const int32_t bn = __shfl_up(n, off, 64);
        const int bf = __shfl_up((int)f, off, 64);
        if (lane >= off) {
          if (!f) { a = ba + a; n = bn + n; }
          f = f || bf != 0;
        }
      }
      if (lane == 63) { sh.wsum[b][wave] = a; sh.wsteps[b][wave] = n; sh.wflag[b][wave] = (int32_t)f; }
      __syncthreads();
      // what the group that reaches into this thread has gathered before it: the carry of the tiles before (walk-on),
      // the waves before this one in wave order, then the lanes before this one
      double cs = 0.0;
      int32_t cn = 0, cm = kCumNoPos;
      if (!home) { cs = sh.csum[b]; cn = sh.csteps[b]; cm = sh.cmin[b]; }
      for (int w = 0; w < wave; ++w) {
        if (sh.wflag[b][w]) { cs = sh.wsum[b][w]; cn = sh.wsteps[b][w]; }
        else { cs = cs + sh.wsum[b][w]; cn += sh.wsteps[b][w]; }
      }
      double cur = __shfl_up(a, 1, 64);
      int32_t cnt = __shfl_up(n, 1, 64);
      const int curf = __shfl_up((int)f, 1, 64);
      if (lane == 0) { cur = cs; cnt = cn; }
      else if (!curf) { cur = cs + cur; cnt = cn + cnt; }

      int32_t stp[kPredRowsPerThread];                         // participating positions of the group before position i
      uint32_t above = 0u;                                      // bit i: position i takes part and its run is > the level
      int32_t m = kCumNoPos;                                    // the first such position since the last group start
#pragma unroll
      for (int i = 0; i < kPredRowsPerThread; ++i) {
        const int q = tid * per + i;
        if (flags & (CUM_START << i)) { cur = 0.0; cnt = 0; m = kCumNoPos; }
        stp[i] = cnt;
        if (row[i] >= 0) {
          cur += (double)x[i];
          ++cnt;
          if (has_level && cur > (home ? sh.lvl[q] : wlevel)) {  // strict, f64, false for NaN
            above |= 1u << i;
            if (m == kCumNoPos) m = (int32_t)(base + q);
          }
        }
        if (flags & (CUM_STORED << i)) {
          if (o.running) o.running[s * R + base + q] = cur;
          if (flags & (CUM_END << i)) o.total[s * (int64_t)G + (home ? sh.grp[q] : gw)] = cur;
        }
      }
      if (carry_to) { sh.csum[b ^ 1] = cur; sh.csteps[b ^ 1] = cnt; }

      if (has_level) {                                          // block-uniform
        // second segmented scan, int32 with min: has the group that reaches into this thread crossed before it?
        bool f2 = f0;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const int32_t bm = __shfl_up(m, off, 64);
          const int bf = __shfl_up((int)f2, off, 64);
          if (lane >= off) {
            if (!f2) m = min(bm, m);
            f2 = f2 || bf != 0;
          }
        }
        if (lane == 63) sh.wmin[b][wave] = m;
        __syncthreads();
        for (int w = 0; w < wave; ++w) cm = sh.wflag[b][w] ? sh.wmin[b][w] : min(cm, sh.wmin[b][w]);
        int32_t curm = __shfl_up(m, 1, 64);
        const int curf2 = __shfl_up((int)f2, 1, 64);
        if (lane == 0) curm = cm;
        else if (!curf2) curm = min(cm, curm);
#pragma unroll
        for (int i = 0; i < kPredRowsPerThread; ++i) {
          const int q = tid * per + i;
          if (flags & (CUM_START << i)) curm = kCumNoPos;
          const bool crosses = ((above >> i) & 1u) && curm == kCumNoPos;     // the group's crossing position
          const bool censored = (flags & (CUM_END << i)) && !crosses && curm == kCumNoPos;   // never crossed
          if ((above >> i) & 1u) {
            if (o.above_count) atomicAdd(&o.above_count[row[i]], 1u);
            if (crosses) {
              curm = (int32_t)(base + q);
              if (o.cross_count) atomicAdd(&o.cross_count[row[i]], 1u);
            }
          }
          if (crosses || censored) {
            const int64_t idx = s * (int64_t)G + (home ? sh.grp[q] : gw);
            if (o.cross_step) o.cross_step[idx] = (double)(crosses ? stp[i] : stp[i] + (row[i] >= 0 ? 1 : 0));
            if (o.cross_row) o.cross_row[idx] = crosses ? row[i] : -1;
          }
        }
        if (carry_to) sh.cmin[b ^ 1] = curm;
      }

      if (!walk) break;
      base += kPredTile;                                        // walk: the home tile is a whole one
      if (base >= wend) break;
    }
  }
}

}  // namespace bnf
