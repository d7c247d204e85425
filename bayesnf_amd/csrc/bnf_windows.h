// bnf_windows.h -- moving-window totals of the posterior-predictive sample paths (bnf_predictive_group_windows): per
// (path s, group g) the f64 sum of the draws over the last w positions at every position, the largest such sum over the
// group's full-length windows with the row at which it is first reached and, against a per-group threshold, the number
// of full-length windows above it, without materialising the S x R draws.  The definitions are the contract above the
// entry point in include/bnf.h.  A sibling of k_predictive_group_cumulative (bnf_cumulative.h), whose structure carries
// over: the same draws (predictive_draw<OBS>, pred_component), the same CSR input, the same tiling of the POSITION axis
// into kPredTile = 1024, thread t -> the 4 CONSECUTIVE positions 4t .. 4t + 3, a block OWNS the groups that START in its
// tile and walks on over the following tiles for the group that leaves through the far edge.  ONE kernel, no work
// buffer, no combine pass, and no workgroup ever waits for another.
//
// What is scanned: d[p] = x[p] - x[p - w], the second term 0 before the group's start and at an entry that takes no
// part; the inclusive segmented scan of d from the group's start is the clipped window sum.  A NaN draw enters the f64
// scan as 0 and an int32 rides the same scan: +1 where a NaN draw enters the window, -1 where it leaves.  While that
// count is positive the window is NaN; once the NaN has left, the sum is finite again (a sliding sum of the NaN itself
// would never recover).  Draws are taken to be finite or NaN: an infinite draw would leave inf - inf behind.
//
// Where x[p - w] comes from.  predictive_draw(seed, path, row) is a pure function, so the draw that leaves can be had
// again anywhere.  The block keeps the draws of the chunk it works on AND of the chunk before in LDS (2 x 4 KB of
// floats, by the parity of the chunk counter, one barrier):
//   * p - w in the chunk                     -> LDS.  In the home tile always: a window is clipped at the group's start,
//                                               and the groups a block owns start in its tile.
//   * p - w in the chunk before (walk-on)    -> LDS, the other buffer.  A walk-on chunk follows a whole one.
//   * p - w further back (walk-on, w > 1024) -> drawn again, once.
// So a position costs one draw for w <= 1024 and at most two beyond.  (With the chunk's own draws alone the first w
// positions of every walk-on chunk would be drawn again by the chunk's first lanes while three waves wait at the
// barrier: for w = 7 that is a second draw's latency per chunk for 7 values.  The second buffer costs 4 KB.)
//
// Per path and chunk: (1) every thread draws its 4 positions into LDS; barrier; (2) it gathers the 4 leaving draws
// (LDS, or the second draw site, which a home tile never enters); (3) segmented __shfl_up scan of (f64 sum, NaN count,
// "a group starts here") over the wave, the 4 wave totals through LDS, joined in wave order, the carry of the chunk
// before (walk-on) as the left operand; the thread folds its positions on top of the exclusive result: the window at
// every position, stored to `window`, compared with the threshold (exceed_count); (4) a second segmented scan of
// (value, position, count above) under the total order of bnf_extremes.h (value descending, position ascending; a NaN
// window is no candidate) gives at the group's last position the peak, its row and the count, carried through the walk
// like the sum.  CANDIDATES are the participating positions p with p - o0 + 1 >= min(w, o1 - o0).
//
// Order of the f64 additions (it follows the tiling, so it may depend on where a group lies on the position axis, and
// on nothing else): the difference d first; inside a thread left to right; lanes by the shift-up scan (left operand =
// the earlier lanes); waves in wave order; the carry of the earlier chunks is the left operand of the chunk's prefix.
// NB / ZINB: every partial sum is an integer below 2^53 in magnitude, the order plays no part.  NORMAL: a window is a
// sum of up to 2 n terms from the group's start, |error| <= 2 n u sum |x| over the n participating positions so far.
// LDS: the home tile's (row, group, threshold: 16 bytes per position) + flags = 17,408 bytes, the draws 8,192, the wave
// totals and carries 312.  No floating-point atomics.  peak_count[r], exceed_count[r] are integer atomicAdd (order-free).
#pragma once

#include "bnf_sampling.h"

namespace bnf {

constexpr int32_t kWinNoPos = 0x7fffffff;      // no CSR position is this large: R <= 2^31 - 1

struct WinOut {
  const double* threshold;  // (G,) or null
  double* peak;             // (S, G)
  int32_t* peak_row;        // (S, G) or null
  double* window;           // (S, R) by position, or null
  double* count;            // (S, G) or null
  uint32_t* peak_count;     // (R,) or null
  uint32_t* exceed_count;   // (R,) or null
};

struct WinShared {
  double thr[kPredTile];    // the home tile: threshold of the position's group
  int32_t row[kPredTile];   //   table row, -1: takes no part or is not this block's
  int32_t grp[kPredTile];   //   group
  float x[2][kPredTile];    // the draws of this chunk and of the one before, by position; 0 where none takes part
  uint32_t flags[256];      // the home tile, per thread: WIN_* << i for its position i
  double wsum[2][4];        // wave totals since the last group start in the wave: sum of d,
  double wpeak[2][4];       //   best candidate window
  double csum[2], cpeak[2]; // carry of a group that walks on: its state at the end of the chunk before
  int32_t wnan[2][4], wflag[2][4], wpos[2][4], wcnt[2][4];
  int32_t cnan[2], cpos[2], ccnt[2];
};

// per position i of a thread: a group starts here / ends here / the position is this block's (its window is stored) /
// it ends a full-length window and takes part / the position w before it lies in its group
enum : uint32_t { WIN_START = 1u, WIN_END = 1u << 4, WIN_STORED = 1u << 8, WIN_CAND = 1u << 12, WIN_LEAVE = 1u << 16 };

// the total order of bnf_extremes.h on (window, position): b beats a iff it is larger, or equal and earlier
__device__ __forceinline__ void win_join(double& v, int32_t& pos, double bv, int32_t bpos) {
  if (bv > v || (bv == v && bpos < pos)) { v = bv; pos = bpos; }
}

template <int OBS>
__global__ __launch_bounds__(256) void k_predictive_group_windows(
    const float* __restrict__ loc, const float* __restrict__ aux, int32_t M, int64_t R,
    const int32_t* __restrict__ seg_offsets, const int32_t* __restrict__ seg_rows, int32_t G, int64_t S, uint64_t seed,
    int64_t row0, int64_t sample0, const double* __restrict__ cum, int32_t window, WinOut o) {
  __shared__ __attribute__((aligned(16))) WinShared sh;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t tile0 = (int64_t)blockIdx.x * kPredTile;
  const int64_t tile_end = tile0 + kPredTile < R ? tile0 + kPredTile : R;
  const int n_valid = (int)(tile_end - tile0);
  const bool has_thr = o.threshold != nullptr;
  const int64_t W = window;
  const double kNone = -__builtin_huge_val();

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
      double thr = 0.0;
      if (q < n_valid) {
        const int64_t p = tile0 + q;
        const int32_t g = pred_group_of(seg_offsets, G, p);
        const int64_t o0 = seg_offsets[g], o1 = seg_offsets[g + 1];
        if (o0 >= tile0) {                                       // a group begun in an earlier tile is that tile's
          const int32_t rr = seg_rows[p];
          row = (rr >= 0 && (int64_t)rr < R) ? rr : -1;          // a row outside the table takes no part
          grp = g;
          if (has_thr) thr = o.threshold[g];
          flags |= WIN_STORED << i;
          if (p == o0) flags |= WIN_START << i;
          if (p + 1 == o1) flags |= WIN_END << i;
          const int64_t len = o1 - o0;
          if (row >= 0 && p - o0 + 1 >= (W < len ? W : len)) flags |= WIN_CAND << i;
          if (p - W >= o0) flags |= WIN_LEAVE << i;
        }
      }
      sh.row[q] = row; sh.grp[q] = grp; sh.thr[q] = thr;
    }
    sh.flags[tid] = flags;
  }
  // the group that holds the tile's last position: if it starts here and goes on, this block walks on to its end
  const int32_t gw = pred_group_of(seg_offsets, G, tile_end - 1);
  const int64_t wstart = seg_offsets[gw];
  int64_t wend = seg_offsets[gw + 1];
  if (wend > R) wend = R;
  const bool walk = wstart >= tile0 && wend > tile_end;                              // block-uniform
  const double wthr = (walk && has_thr) ? o.threshold[gw] : 0.0;
  const int64_t wneed = W < wend - wstart ? W : wend - wstart;   // positions a full-length window of that group holds

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
        // the group's last piece: its positions spread over the threads, 1 to 4 consecutive ones each
        if (wend - base < kPredTile) per = (int)((wend - base + 255) >> 8);
#pragma unroll
        for (int i = 0; i < kPredRowsPerThread; ++i) {
          const int64_t p = base + tid * per + i;
          row[i] = -1;
          if (i < per && p < wend) {
            const int32_t rr = seg_rows[p];
            row[i] = (rr >= 0 && (int64_t)rr < R) ? rr : -1;
            flags |= WIN_STORED << i;
            if (p + 1 == wend) flags |= WIN_END << i;
            if (row[i] >= 0 && p - wstart + 1 >= wneed) flags |= WIN_CAND << i;
            if (p - W >= wstart) flags |= WIN_LEAVE << i;
          }
        }
      }
      // this thread holds the chunk's last position and its group walks on: it hands the carry to the next chunk
      const bool carry_to = walk && tid == 255 && base + kPredTile < wend;

      // (1) the chunk's draws, kept in LDS by position for the windows they leave later
#pragma unroll 1
      for (int i = 0; i < per; ++i)
        sh.x[b][tid * per + i] =
            row[i] >= 0 ? predictive_draw<OBS>(seed, sg, (uint64_t)(row0 + row[i]), lrow[row[i]], a0, a1, a2) : 0.f;
      __syncthreads();

      // (2) the draw that leaves the window of every position: this chunk's or the chunk's before from LDS; further back
      // (walk-on only: a home tile's windows are clipped inside it) its row, to be drawn again
      float xl[kPredRowsPerThread];
      int32_t back[kPredRowsPerThread];
#pragma unroll
      for (int i = 0; i < kPredRowsPerThread; ++i) {
        xl[i] = 0.f;
        back[i] = -1;
        if (flags & (WIN_LEAVE << i)) {
          const int64_t ql = base + tid * per + i - W;          // >= the group's start, which is >= tile0
          if (ql >= base) xl[i] = sh.x[b][ql - base];
          else if (ql >= base - kPredTile) xl[i] = sh.x[b ^ 1][ql - base + kPredTile];
          else {
            const int32_t rr = seg_rows[ql];
            back[i] = (rr >= 0 && (int64_t)rr < R) ? rr : -1;
          }
        }
      }
      if (!home && W > kPredTile) {                             // block-uniform
#pragma unroll 1
        for (int i = 0; i < kPredRowsPerThread; ++i)
          if (back[i] >= 0)
            xl[i] = predictive_draw<OBS>(seed, sg, (uint64_t)(row0 + back[i]), lrow[back[i]], a0, a1, a2);
      }

      // (3) d = entering - leaving draw, a NaN as 0 with its count; the thread's sums since the last group start in it
      double d[kPredRowsPerThread];
      int32_t dn[kPredRowsPerThread];
      double a = 0.0;
      int32_t n = 0;
      const bool f0 = (flags & 0xfu) != 0u;
#pragma unroll
      for (int i = 0; i < kPredRowsPerThread; ++i) {
        const float xe = i < per ? sh.x[b][tid * per + i] : 0.f;   // written by this thread
        const bool ne = xe != xe, nl = xl[i] != xl[i];
        d[i] = (double)(ne ? 0.f : xe) - (double)(nl ? 0.f : xl[i]);
        dn[i] = (int32_t)ne - (int32_t)nl;
        if (flags & (WIN_START << i)) { a = 0.0; n = 0; }
        a += d[i];
        n += dn[i];
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
      if (lane == 63) { sh.wsum[b][wave] = a; sh.wnan[b][wave] = n; sh.wflag[b][wave] = (int32_t)f; }
      __syncthreads();
      // what the group that reaches into this thread has gathered before it: the carry of the chunks before (walk-on),
      // the waves before this one in wave order, then the lanes before this one
      double cs = 0.0;
      int32_t cn = 0;
      if (!home) { cs = sh.csum[b]; cn = sh.cnan[b]; }
      for (int w = 0; w < wave; ++w) {
        if (sh.wflag[b][w]) { cs = sh.wsum[b][w]; cn = sh.wnan[b][w]; }
        else { cs = cs + sh.wsum[b][w]; cn += sh.wnan[b][w]; }
      }
      double cur = __shfl_up(a, 1, 64);
      int32_t cnt = __shfl_up(n, 1, 64);
      const int curf = __shfl_up((int)f, 1, 64);
      if (lane == 0) { cur = cs; cnt = cn; }
      else if (!curf) { cur = cs + cur; cnt = cn + cnt; }

      double win[kPredRowsPerThread];
      uint32_t ok = 0u, above = 0u;         // bit i: position i is a candidate with a window that is not NaN / > threshold
      double pv = kNone;                    // the thread's best candidate since the last group start inside it,
      int32_t pp = kWinNoPos, pc = 0;       //   its position, and the candidates above the threshold
#pragma unroll
      for (int i = 0; i < kPredRowsPerThread; ++i) {
        const int q = tid * per + i;
        if (flags & (WIN_START << i)) { cur = 0.0; cnt = 0; pv = kNone; pp = kWinNoPos; pc = 0; }
        cur += d[i];
        cnt += dn[i];
        win[i] = cnt > 0 ? __builtin_nan("") : cur;
        if ((flags & (WIN_STORED << i)) && o.window) o.window[s * R + base + q] = win[i];
        if ((flags & (WIN_CAND << i)) && cnt <= 0) {
          ok |= 1u << i;
          win_join(pv, pp, cur, (int32_t)(base + q));
          if (has_thr && cur > (home ? sh.thr[q] : wthr)) {      // strict, f64
            above |= 1u << i;
            ++pc;
            if (o.exceed_count) atomicAdd(&o.exceed_count[row[i]], 1u);
          }
        }
      }
      if (carry_to) { sh.csum[b ^ 1] = cur; sh.cnan[b ^ 1] = cnt; }

      // (4) second segmented scan: the best candidate and the count above since the group's start
      bool f2 = f0;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const double bv = __shfl_up(pv, off, 64);
        const int32_t bp = __shfl_up(pp, off, 64);
        const int32_t bc = __shfl_up(pc, off, 64);
        const int bf = __shfl_up((int)f2, off, 64);
        if (lane >= off) {
          if (!f2) { win_join(pv, pp, bv, bp); pc += bc; }
          f2 = f2 || bf != 0;
        }
      }
      if (lane == 63) { sh.wpeak[b][wave] = pv; sh.wpos[b][wave] = pp; sh.wcnt[b][wave] = pc; }
      __syncthreads();
      double cv = kNone;
      int32_t cp = kWinNoPos, cc = 0;
      if (!home) { cv = sh.cpeak[b]; cp = sh.cpos[b]; cc = sh.ccnt[b]; }
      for (int w = 0; w < wave; ++w) {
        if (sh.wflag[b][w]) { cv = sh.wpeak[b][w]; cp = sh.wpos[b][w]; cc = sh.wcnt[b][w]; }
        else { win_join(cv, cp, sh.wpeak[b][w], sh.wpos[b][w]); cc += sh.wcnt[b][w]; }
      }
      double ev = __shfl_up(pv, 1, 64);
      int32_t ep = __shfl_up(pp, 1, 64), ec = __shfl_up(pc, 1, 64);
      const int evf = __shfl_up((int)f2, 1, 64);
      if (lane == 0) { ev = cv; ep = cp; ec = cc; }
      else if (!evf) { win_join(ev, ep, cv, cp); ec += cc; }
#pragma unroll
      for (int i = 0; i < kPredRowsPerThread; ++i) {
        const int q = tid * per + i;
        if (flags & (WIN_START << i)) { ev = kNone; ep = kWinNoPos; ec = 0; }
        if ((ok >> i) & 1u) win_join(ev, ep, win[i], (int32_t)(base + q));
        ec += (int32_t)((above >> i) & 1u);
        if (flags & (WIN_END << i)) {                            // the group's last position: its results
          const int64_t idx = s * (int64_t)G + (home ? sh.grp[q] : gw);
          const bool none = ep == kWinNoPos;
          const int32_t prow = none ? -1 : seg_rows[ep];         // a candidate takes part: a row of the table
          o.peak[idx] = none ? __builtin_nan("") : ev;
          if (o.peak_row) o.peak_row[idx] = prow;
          if (o.count) o.count[idx] = (double)ec;
          if (o.peak_count && !none) atomicAdd(&o.peak_count[prow], 1u);
        }
      }
      if (carry_to) { sh.cpeak[b ^ 1] = ev; sh.cpos[b ^ 1] = ep; sh.ccnt[b ^ 1] = ec; }

      if (!walk) break;
      base += kPredTile;                                        // walk: the home tile is a whole one
      if (base >= wend) break;
    }
  }
}

}  // namespace bnf
