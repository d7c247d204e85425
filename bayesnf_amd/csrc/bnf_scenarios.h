// bnf_scenarios.h -- a few representative joint scenarios out of an ensemble of sample paths (bnf_sample_distances,
// bnf_scenario_select): fast forward selection (Heitsch & Roemisch 2003), which greedily picks the paths that minimise the
// Kantorovich distance between the S equally likely paths and the chosen ones with optimally redistributed mass.  Input
// x (S, C) f64 row-major: S sample paths of C columns, as bnf_predictive_group_sums writes them.  Everything is f64; no
// floating-point atomics; every sum is in an order the shapes fix, so two calls give the same bits.
//
// k_scn_distances<P, SCALED>: dist (S, S), dist[s][t] = sum_c |term_c| (P = 1) or sqrt(sum_c term_c * term_c) (P = 2),
//   term_c = x_sc - x_tc, with a scale (x_sc - x_tc) / scale_c: ONE IEEE division of the difference, so that a total of
//   1e9 with a spread of 10 loses nothing and the error of a term is relative to the term.  The columns that take part are
//   those whose y_c is finite (all of them without y); the sum of a cell runs over them in ascending order as ONE
//   sequential f64 sum, a product never contracted into the addition that follows (fp contract(off)).  The scheme is
//   k_energy_pairs': the S x S pairs are cut into tiles of 64 x 64 paths, only the tiles on and above the diagonal run,
//   the columns stream through LDS in chunks of 32 stored [column][path] with a pitch of 65 doubles, a thread owns 4 x 4
//   pairs (rows ty + 16 i against rows tx + 16 j).  A skipped column (and a row past S) is staged as 0.0 on both sides
//   with a divisor of 1.0: it adds +0.0 to a sum that is >= +0.0 or NaN, which changes no bit -- so a cell's bits depend
//   on its two paths and the participating columns only, not on S, the other paths or the tile geometry.  The terms of
//   (s, t) and (t, s) differ in sign alone and |.|, the square and the division are sign-symmetric: the diagonal tiles
//   compute both cells, the others store one value twice.  The diagonal is a cell like any other: +0.0, or NaN for a
//   path with a NaN in a participating column (which is NaN in its whole row and column).
//   The stores: the 64 x 64 tile of results is staged in LDS (the chunk buffers' own 64 * 65 doubles, after a barrier),
//   pitch 65, and written out row by row, a wave storing 64 consecutive doubles (512 B) of one row of dist; the mirrored
//   tile reads the staged tile down its columns (lane l at double 65 l + r: bank pairs 2 l mod 64, distinct within each
//   32-lane half, the groups of an 8-byte LDS read) and stores rows of dist just as wide -- no stride-S scatter.
//   Every LDS cell read has been written by this kernel: the chunk buffers are filled whole (data, or 0.0) before every
//   chunk's reads, and all 64 x 64 tile cells are written before the stores read them.
// k_scn_ydist<P, SCALED>: ydist[s] = the same distance between path s and y, the same sequential sum (a y equal to path t
//   gives the bits of dist[s][t]); 64 paths per workgroup, the columns staged the same way.
//
// bnf_scenario_select on a symmetric dist (S, S), read BY ROWS throughout (dist[u][s] for dist[s][u]: the candidate sums
// stream).  work = dmin (S f64) | z (S f64) | taken (S int32, later the assignment) | flag, pick (2 int32).
//   k_scn_init     dmin = +inf, taken = 0, flag |= any NaN cell of dist (an integer atomicOr; the flag was zeroed on the stream)
//   step i = 1..k, enqueued back to back; the pick of a step stays on the device:
//   k_scn_sums     one workgroup of 256 threads per candidate u not yet taken: z[u] = sum_s min(dmin_s, dist[u][s]).
//                  THE ORDER: thread t adds s = t, t + 256, t + 512, ... in that order from 0.0; the wave butterfly
//                  v += shfl_xor(v, off), off = 32, 16, 8, 4, 2, 1; then the four waves in order ((w0 + w1) + w2) + w3.
//                  It depends on S alone.  tests/scenarios_ref.py scenarios_kernel_form restates it.
//   k_scn_pick     one workgroup: u_i = the untaken u with the smallest z[u], the lowest index among equal ones ((z, u)
//                  compared lexicographically at every stage of the reduction); chosen[i - 1] = u_i,
//                  objective[i - 1] = z[u_i] / (double)S -- the very sum that won, divided once; taken[u_i] = 1;
//                  dmin_s = min(dmin_s, dist[u_i][s])
//   k_scn_assign   assign[s] = the smallest j with dist[chosen[j]][s] == dmin_s, nearest[s] = dmin_s
//   k_scn_finish   prob[j] = #{s : assign[s] = j} / (double)S (integer counts); with ydist: obs_nearest = the earliest j that
//                  minimises ydist[chosen[j]], obs[0] that distance, obs[1] = #{s : nearest_s <= obs[0]} / S,
//                  obs[2] = #{s : nearest_s < obs[0]} / S
//   With the flag set every kernel writes -1 / NaN instead; the host never waits for the flag.
#pragma once

#include "bnf_sampling.h"
#include "bnf_totals.h"

namespace bnf {

constexpr int kScnMaxSamples = BNF_SCENARIO_MAX_SAMPLES;
constexpr int kScnTile = 64;                        // paths per side of a pair tile
constexpr int kScnCols = 32;                        // columns per LDS chunk
constexpr int kScnPitch = kScnTile + 1;
constexpr int kScnThreads = 256;
static_assert(2 * kScnCols * kScnPitch == kScnTile * kScnPitch, "the result tile is staged in the two chunk buffers");

constexpr int64_t scenario_tiles(int64_t S) { return (S + kScnTile - 1) / kScnTile; }
// dmin and z (S f64 each), taken / assignment (S int32), flag and pick (2 int32), the end padded to 8 bytes
constexpr size_t scenario_work_bytes(int64_t S) { return (size_t)(20 * S + 16); }

struct ScnWork {
  double* dmin;
  double* z;
  int32_t* taken;
  int32_t* flag;      // flag[0]: a NaN cell in dist; flag[1]: the pick of the last step
};
inline ScnWork scenario_work(void* work, int64_t S) {
  ScnWork w;
  w.dmin = (double*)work;
  w.z = w.dmin + S;
  w.taken = (int32_t*)(w.z + S);
  w.flag = w.taken + S + (S & 1);                   // 8-byte aligned
  return w;
}

template <int P, bool SCALED>
__device__ __forceinline__ double scn_accumulate(double acc, double a, double b, double sc) {
#pragma clang fp contract(off)
  double d = a - b;
  if (SCALED) d = d / sc;
  if (P == 1) return acc + fabs(d);
  const double q = d * d;
  return acc + q;
}

// grid (nT, nT): tile (ti = blockIdx.y, tj = blockIdx.x), the tiles below the diagonal leave at once.
template <int P, bool SCALED>
__global__ __launch_bounds__(256) void k_scn_distances(const double* __restrict__ x, int64_t S, int64_t G,
                                                       const double* __restrict__ scale, const double* __restrict__ y,
                                                       double* __restrict__ dist) {
  const int64_t ti = blockIdx.y, tj = blockIdx.x;
  if (tj < ti) return;
  __shared__ __attribute__((aligned(16))) double sm[kScnTile * kScnPitch];
  __shared__ double ssc[kScnCols];
  double* sa_ = sm;
  double* sb_ = sm + kScnCols * kScnPitch;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int lcol = tid & (kScnCols - 1), lrow = tid >> 5;          // staging: 32 columns x 8 paths per pass
  const int64_t a0 = ti * kScnTile, b0 = tj * kScnTile;
  double acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;

  for (int64_t cb = 0; cb < G; cb += kScnCols) {
    __syncthreads();                                   // the previous chunk's reads are done
    const int64_t c = cb + lcol;
    const bool cok = c < G && (!y || totals_finite(y[c < G ? c : 0]));
    if (SCALED && lrow == 0) ssc[lcol] = cok ? scale[c] : 1.0;
#pragma unroll
    for (int p = 0; p < kScnTile / 8; ++p) {
      const int r = lrow + 8 * p;
      const int64_t ra = a0 + r, rb = b0 + r;
      sa_[lcol * kScnPitch + r] = (cok && ra < S) ? x[ra * G + c] : 0.0;
      sb_[lcol * kScnPitch + r] = (cok && rb < S) ? x[rb * G + c] : 0.0;
    }
    __syncthreads();
#pragma unroll 4
    for (int cc = 0; cc < kScnCols; ++cc) {
      double av[4], bv[4];
      const double sc = SCALED ? ssc[cc] : 1.0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        av[i] = sa_[cc * kScnPitch + ty + 16 * i];
        bv[i] = sb_[cc * kScnPitch + tx + 16 * i];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = scn_accumulate<P, SCALED>(acc[i][j], av[i], bv[j], sc);
    }
  }
  __syncthreads();                                     // the last chunk's reads are done: sm becomes the result tile
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) sm[(ty + 16 * i) * kScnPitch + tx + 16 * j] = P == 2 ? sqrt(acc[i][j]) : acc[i][j];
  __syncthreads();
  const int lane = tid & 63, wv = tid >> 6;
  for (int r = wv; r < kScnTile; r += 4) {             // row a0 + r of dist, columns b0 ..: 64 consecutive doubles a wave
    const int64_t ra = a0 + r, rb = b0 + lane;
    if (ra < S && rb < S) dist[ra * S + rb] = sm[r * kScnPitch + lane];
  }
  if (tj != ti)
    for (int r = wv; r < kScnTile; r += 4) {           // the mirrored tile: row b0 + r of dist, columns a0 ..
      const int64_t rb = b0 + r, ra = a0 + lane;
      if (rb < S && ra < S) dist[rb * S + ra] = sm[lane * kScnPitch + r];
    }
}

// grid (nT): ydist[s] for the 64 paths of tile blockIdx.x; the first 64 threads own one path each
template <int P, bool SCALED>
__global__ __launch_bounds__(256) void k_scn_ydist(const double* __restrict__ x, int64_t S, int64_t G,
                                                   const double* __restrict__ scale, const double* __restrict__ y,
                                                   double* __restrict__ ydist) {
  __shared__ __attribute__((aligned(16))) double sa_[kScnCols * kScnPitch];
  __shared__ double ssc[kScnCols];
  __shared__ double sy[kScnCols];
  const int tid = threadIdx.x;
  const int lcol = tid & (kScnCols - 1), lrow = tid >> 5;
  const int64_t a0 = (int64_t)blockIdx.x * kScnTile;
  double acc = 0.0;
  for (int64_t cb = 0; cb < G; cb += kScnCols) {
    __syncthreads();
    const int64_t c = cb + lcol;
    const double yv = c < G ? y[c] : 0.0;
    const bool cok = c < G && totals_finite(yv);
    if (lrow == 0) {
      sy[lcol] = cok ? yv : 0.0;
      ssc[lcol] = (SCALED && cok) ? scale[c] : 1.0;
    }
#pragma unroll
    for (int p = 0; p < kScnTile / 8; ++p) {
      const int r = lrow + 8 * p;
      const int64_t ra = a0 + r;
      sa_[lcol * kScnPitch + r] = (cok && ra < S) ? x[ra * G + c] : 0.0;
    }
    __syncthreads();
    if (tid < kScnTile)
      for (int cc = 0; cc < kScnCols; ++cc)
        acc = scn_accumulate<P, SCALED>(acc, sa_[cc * kScnPitch + tid], sy[cc], ssc[cc]);
  }
  if (tid < kScnTile && a0 + tid < S) ydist[a0 + tid] = P == 2 ? sqrt(acc) : acc;
}

template <int P, bool SCALED>
inline void launch_scn_distances(hipStream_t stream, const double* x, int64_t S, int64_t G, const double* scale,
                                 const double* y, double* dist, double* ydist) {
  const int64_t nT = scenario_tiles(S);
  hipLaunchKernelGGL((k_scn_distances<P, SCALED>), dim3((unsigned)nT, (unsigned)nT), dim3(256), 0, stream, x, S, G, scale,
                     y, dist);
  if (ydist)
    hipLaunchKernelGGL((k_scn_ydist<P, SCALED>), dim3((unsigned)nT), dim3(256), 0, stream, x, S, G, scale, y, ydist);
}

// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_scn_init(const double* __restrict__ dist, int64_t S, ScnWork w) {
  const int64_t n = S * S, stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int any = 0;
  for (int64_t i = g; i < n; i += stride) {
    const double v = dist[i];
    any |= v != v ? 1 : 0;
  }
  for (int64_t s = g; s < S; s += stride) {
    w.dmin[s] = INFINITY;
    w.taken[s] = 0;
  }
  any = __syncthreads_or(any);
  if (threadIdx.x == 0 && any) atomicOr(w.flag, 1);
}

__device__ __forceinline__ int32_t wave_sum_i32(int32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// ((z, u) < (bz, bu)) lexicographically: the smaller sum, the lower index among equal ones
__device__ __forceinline__ bool scn_before(double z, int32_t u, double bz, int32_t bu) {
  return z < bz || (z == bz && u < bu);
}

// grid (S): candidate u = blockIdx.x
__global__ __launch_bounds__(256) void k_scn_sums(const double* __restrict__ dist, int64_t S, ScnWork w) {
  __shared__ double wsum[4];
  const int64_t u = blockIdx.x;
  if (w.flag[0] || w.taken[u]) return;
  const int tid = threadIdx.x;
  const double* row = dist + u * S;
  double acc = 0.0;
  for (int64_t s = tid; s < S; s += kScnThreads) acc += fmin(w.dmin[s], row[s]);
  acc = wave_sum_f64(acc);
  if ((tid & 63) == 0) wsum[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) w.z[u] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// one workgroup: the pick of step `step` (0-based) and the update of dmin
__global__ __launch_bounds__(256) void k_scn_pick(const double* __restrict__ dist, int64_t S, int32_t step, ScnWork w,
                                                  int32_t* __restrict__ chosen, double* __restrict__ objective) {
  __shared__ double wz[4];
  __shared__ int32_t wu[4];
  __shared__ int32_t pick_sm;
  const int tid = threadIdx.x;
  if (w.flag[0]) {
    if (tid == 0) {
      chosen[step] = -1;
      objective[step] = __builtin_nan("");
    }
    return;
  }
  double bz = INFINITY;
  int32_t bu = 0x7fffffff;
  for (int32_t u = tid; u < S; u += kScnThreads)
    if (!w.taken[u]) {
      double z = w.z[u];
      z = z != z ? INFINITY : z;                        // (a dist that is not ours: -inf beside +inf; never an index past S)
      if (scn_before(z, u, bz, bu)) { bz = z; bu = u; }
    }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double oz = __shfl_xor(bz, off, 64);
    const int32_t ou = __shfl_xor(bu, off, 64);
    if (scn_before(oz, ou, bz, bu)) { bz = oz; bu = ou; }
  }
  if ((tid & 63) == 0) { wz[tid >> 6] = bz; wu[tid >> 6] = bu; }
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < 4; ++k)
      if (scn_before(wz[k], wu[k], bz, bu)) { bz = wz[k]; bu = wu[k]; }
    pick_sm = bu;                                       // < S: step < S leaves an untaken candidate
    chosen[step] = bu;
    objective[step] = bz / (double)S;
    w.taken[bu] = 1;
    w.flag[1] = bu;
  }
  __syncthreads();
  const double* row = dist + (int64_t)pick_sm * S;
  for (int64_t s = tid; s < S; s += kScnThreads) w.dmin[s] = fmin(w.dmin[s], row[s]);
}

// grid (ceil(S / 256)): one thread per path; the assignment goes to work (taken is free now) and to assign
__global__ __launch_bounds__(256) void k_scn_assign(const double* __restrict__ dist, int64_t S, int32_t k, ScnWork w,
                                                    const int32_t* __restrict__ chosen, int32_t* __restrict__ assign,
                                                    double* __restrict__ nearest) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  int32_t a = -1;
  double d = __builtin_nan("");
  if (!w.flag[0]) {
    d = w.dmin[s];
    for (int32_t j = 0; j < k; ++j)
      if (dist[(int64_t)chosen[j] * S + s] == d) { a = j; break; }
  }
  w.taken[s] = a;
  if (assign) assign[s] = a;
  if (nearest) nearest[s] = d;
}

// grid (k + 1): workgroup j < k counts the paths of scenario j; workgroup k scores the observed vector (ydist or NULL)
__global__ __launch_bounds__(256) void k_scn_finish(int64_t S, int32_t k, ScnWork w, const int32_t* __restrict__ chosen,
                                                    const double* __restrict__ ydist, double* __restrict__ prob,
                                                    int32_t* __restrict__ obs_nearest, double* __restrict__ obs) {
  __shared__ int32_t wn[8];
  __shared__ double wz[4];
  __shared__ int32_t wu[4];
  __shared__ double d0_sm;
  const int tid = threadIdx.x;
  const int32_t j = blockIdx.x;
  const bool bad = w.flag[0] != 0;
  const double nan_ = __builtin_nan("");
  if (j < k) {
    int32_t n = 0;
    if (!bad)
      for (int64_t s = tid; s < S; s += kScnThreads) n += w.taken[s] == j ? 1 : 0;
    n = wave_sum_i32(n);
    if ((tid & 63) == 0) wn[tid >> 6] = n;
    __syncthreads();
    if (tid == 0) prob[j] = bad ? nan_ : (double)(wn[0] + wn[1] + wn[2] + wn[3]) / (double)S;
    return;
  }
  if (!ydist) return;
  double bz = INFINITY;
  int32_t bu = 0x7fffffff;
  if (!bad)
    for (int32_t i = tid; i < k; i += kScnThreads) {
      const double z = ydist[chosen[i]];
      if (scn_before(z, i, bz, bu)) { bz = z; bu = i; }
    }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double oz = __shfl_xor(bz, off, 64);
    const int32_t ou = __shfl_xor(bu, off, 64);
    if (scn_before(oz, ou, bz, bu)) { bz = oz; bu = ou; }
  }
  if ((tid & 63) == 0) { wz[tid >> 6] = bz; wu[tid >> 6] = bu; }
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < 4; ++i)
      if (scn_before(wz[i], wu[i], bz, bu)) { bz = wz[i]; bu = wu[i]; }
    wu[0] = bu;
    d0_sm = bz;
  }
  __syncthreads();
  const bool none = bad || wu[0] == 0x7fffffff;          // (a ydist of NaN alone: nothing compares below +inf)
  const double d0 = d0_sm;
  int32_t n_le = 0, n_lt = 0;
  if (!none)
    for (int64_t s = tid; s < S; s += kScnThreads) {
      const double v = w.dmin[s];
      n_le += v <= d0 ? 1 : 0;
      n_lt += v < d0 ? 1 : 0;
    }
  n_le = wave_sum_i32(n_le);
  n_lt = wave_sum_i32(n_lt);
  if ((tid & 63) == 0) { wn[tid >> 6] = n_le; wn[4 + (tid >> 6)] = n_lt; }
  __syncthreads();
  if (tid == 0) {
    obs_nearest[0] = none ? -1 : wu[0];
    obs[0] = none ? nan_ : d0;
    obs[1] = none ? nan_ : (double)(wn[0] + wn[1] + wn[2] + wn[3]) / (double)S;
    obs[2] = none ? nan_ : (double)(wn[4] + wn[5] + wn[6] + wn[7]) / (double)S;
  }
}

}  // namespace bnf
