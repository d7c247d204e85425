// bnf_sampling.h -- posterior-predictive sample paths drawn on the device (bnf_predictive_samples /
// bnf_predictive_group_sums): joint draws of the equal-weight mixture over members that `predict` reports
// marginal quantiles of.  What the reference gets from TFP's `.sample()` on its `likelihood_model()`.
//
//   sample path s  : ONE mixture component c_s = floor(u M) for every row, u a Philox draw keyed by (seed, s); with
//                    member weights (the *_weighted entry points) c_s = #{m : cum[m] <= u}, cum their running sum
//   row r of path s: an independent draw from member c_s's distribution at that row
//       NORMAL  N(loc, aux[0])
//       NB      total_count = 1 / aux[1], logits = -log aux[1] - log softplus(loc), drawn as
//               Poisson(Gamma(shape = total_count, scale = e^logits))
//       ZINB    the NB, replaced by 0 with probability aux[2]
//
// Counter-based, no state: the value at (s, r) is a pure function of (seed, s, GLOBAL row r, loc[c_s, r], aux[c_s]).
// Launch geometry, chunk boundaries, the number of samples or rows asked for and the grouping do not enter.
// Philox4x32-10, key = seed, counter
//   component of path s :  c0 = s             c1 = 0   c2 = 0                     c3 = STREAM_PRED_COMPONENT
//   draw at (s, r)      :  c0 = r bits 0..31  c1 = s   c2 = slot << 16 | trial    c3 = STREAM_PRED_DRAW | r bits 32..55 << 8
//       slot 0 (trial 0): words 0, 1 the Normal draw (Box-Muller), word 2 the zero-inflation uniform
//       slot 1, trial t : Marsaglia-Tsang proposal t: words 0, 1 its normal, word 2 its acceptance uniform, word 3 the
//                         uniform of the shape < 1 boost (the one of the accepted trial is used)
//       slot 2, trial t : Poisson: trial 0 word 0 is the inversion uniform (rate < 10); PTRS proposal t takes words 0, 1
//
// Non-finite parameters: a NaN in loc, or in the aux entry the model reads (NORMAL aux[0]; NB aux[1]; ZINB aux[1], aux[2]),
// of the drawn member gives a NaN draw -- never a count, and the zero inflation does not hide it; a rate beyond the f32
// range gives +inf (in the ZINB, where the inflation has not put its 0).  No finite draw depends on these tests.
//
// Bounded loops: every rejection loop stops after kPredMaxTrials = 64 proposals and takes the last one that lay inside the
// support.  Marsaglia-Tsang rejects with probability < 0.05 (shape >= 1), PTRS with probability < 0.25 (rate >= 10):
// reaching the cap has probability < 0.25^64 = 3e-39 per draw.  The inversion loop ends at k = 64 at the latest
// (P(Poisson(10) > 64) < 1e-28).  No thread can spin.
//
// f32 arithmetic throughout, plain HIP C++.  Contraction of a * b + c into an fma is switched off inside the draw functions:
// the per-row kernel and the group-sum kernel must produce the same bits from the same counters.
#pragma once

#include "bnf_device.h"
#include "../../include/bnf.h"

namespace bnf {

constexpr uint32_t kPredMaxTrials = 64;
constexpr int kPredInvCap = 64;
constexpr float kPredInvRate = 10.f;          // below: sequential inversion; from here on: PTRS
constexpr int kPredTile = BNF_GROUP_TILE;     // CSR positions per tile of the group sums
constexpr int kPredRowsPerThread = 4;
enum : uint32_t { PRED_SLOT_BASE = 0, PRED_SLOT_GAMMA = 1, PRED_SLOT_POISSON = 2 };

__device__ __forceinline__ Philox pred_bits(uint64_t seed, uint32_t s, uint64_t r, uint32_t slot, uint32_t trial) {
  return philox4x32((uint32_t)r, s, (slot << 16) | trial, (uint32_t)STREAM_PRED_DRAW | ((uint32_t)(r >> 32) << 8),
                    (uint32_t)seed, (uint32_t)(seed >> 32));
}

// mixture component of sample path s, equal weights: floor(u M), u = word / 2^32
__device__ __forceinline__ int32_t pred_component(uint64_t seed, uint32_t s, int32_t M) {
  const Philox b = philox4x32(s, 0u, 0u, (uint32_t)STREAM_PRED_COMPONENT, (uint32_t)seed, (uint32_t)(seed >> 32));
  return (int32_t)(((uint64_t)b.v[0] * (uint64_t)(uint32_t)M) >> 32);
}

// weighted form: cum (M,) f64 the running sum of the member weights (nondecreasing, last entry 1), the same Philox word,
// u = word / 2^32 and c_s = #{m : cum[m] <= u} by bisection, clamped to M - 1: whatever cum holds, the result is a
// member, never an index outside loc.  u moves in steps of 2^-32: a member whose weight is below 2^-32 may own no u at
// all and is then never drawn.  cum == nullptr: the integer form above (the equal-weight entry points keep their bits).
__device__ __forceinline__ int32_t pred_component(uint64_t seed, uint32_t s, int32_t M, const double* __restrict__ cum) {
  if (!cum) return pred_component(seed, s, M);
  const Philox b = philox4x32(s, 0u, 0u, (uint32_t)STREAM_PRED_COMPONENT, (uint32_t)seed, (uint32_t)(seed >> 32));
  const double u = (double)b.v[0] * 2.3283064365386963e-10;   // 2^-32, exact
  int32_t lo = 0, hi = M;                                      // cum[m] <= u for m < lo, cum[m] > u for m >= hi
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (cum[mid] <= u) lo = mid + 1; else hi = mid;
  }
  return lo < M - 1 ? lo : M - 1;
}

// log of a Gamma(shape a, scale 1) draw: Marsaglia & Tsang (2000) on shape a (+ 1 where a < 1, then times U^(1/a)).
// Returned as a logarithm: at a = 0.05 the boost U^20 leaves the f32 range for one draw in three.
// v = (1 + c x)^3 is carried as w = v - 1 and the acceptance bound x^2/2 + d - d v + d log v as x^2/2 + d (log1p(w) - w),
// which keeps its O(1) value to ~1e-7 sqrt(d) where the textbook form cancels terms of size d.
__device__ __forceinline__ float pred_log_gamma(uint64_t seed, uint32_t s, uint64_t r, float a) {
#pragma clang fp contract(off)
  const bool boost = a < 1.f;
  const float d = (boost ? a + 1.f : a) - (1.f / 3.f);
  const float c = 1.f / sqrtf(9.f * d);
  float w = 0.f, ub = 0.5f;
#pragma unroll 1
  for (uint32_t t = 0; t < kPredMaxTrials; ++t) {
    const Philox b = pred_bits(seed, s, r, PRED_SLOT_GAMMA, t);
    const float x = std_normal(b.v[0], b.v[1]);
    const float cx = c * x;
    if (cx <= -1.f) continue;                      // v <= 0: outside the support, never taken
    ub = u01_open(b.v[3]);
    w = cx * (3.f + cx * (3.f + cx));
    if (logf(u01_open(b.v[2])) < 0.5f * x * x + d * (log1pf(w) - w)) break;
  }
  float lg = logf(d) + log1pf(w);
  if (boost) lg += logf(ub) / a;
  return lg;
}

// log of the Poisson(lam) mass at k, k >= 10: Stirling's series for lgamma(k + 1) with delta = k - lam taken out,
// delta - k log1p(delta / lam) - log(2 pi k) / 2 - 1 / (12 k) + 1 / (360 k^3)   (next term 1 / (1260 k^5) < 1e-8).
// -lam + k log lam - lgammaf(k + 1) cancels terms of size k log k: an absolute error of ~1 at lam = 10^6 in f32.
__device__ __forceinline__ float pred_poisson_logpmf(float k, float lam, float loglam) {
#pragma clang fp contract(off)
  if (k < 10.f) return -lam + k * loglam - lgammaf(k + 1.f);
  const float delta = k - lam, ik = 1.f / k;
  return delta - k * log1pf(delta / lam) - 0.5f * logf(6.2831853071795865f * k) -
         ik * (1.f / 12.f) * (1.f - ik * ik * (1.f / 30.f));
}

// Poisson(lam) as a float.  lam < 10: sequential inversion of one uniform.  Else Hoermann's transformed rejection
// with squeeze (PTRS, 1993).  Counts above 2^24 come out rounded to the nearest float.  A NaN rate is returned as it is
// (it would fail every compare of the inversion loop and come out as the count 0); the rate +inf comes out as +inf.
__device__ __forceinline__ float pred_poisson(uint64_t seed, uint32_t s, uint64_t r, float lam) {
#pragma clang fp contract(off)
  if (lam != lam) return lam;
  if (!(lam >= kPredInvRate)) {
    const Philox b = pred_bits(seed, s, r, PRED_SLOT_POISSON, 0);
    const float u = u01_open(b.v[0]);
    float p = expf(-lam), cdf = p, k = 0.f;
#pragma unroll 1
    for (int i = 0; i < kPredInvCap && u > cdf; ++i) {
      k += 1.f;
      p *= lam / k;
      cdf += p;
      if (p < 1e-9f && k > lam) break;             // the f32 sum has stopped growing below u: the tail left is < 1e-8
    }
    return k;
  }
  const float slam = sqrtf(lam), loglam = logf(lam);
  const float b_ = 0.931f + 2.53f * slam;
  const float a_ = -0.059f + 0.02483f * b_;
  const float inv_alpha = 1.1239f + 1.1328f / (b_ - 3.4f);
  const float vr = 0.9277f - 3.6224f / (b_ - 2.f);
  float k = floorf(lam), kin = k;
#pragma unroll 1
  for (uint32_t t = 0; t < kPredMaxTrials; ++t) {
    const Philox b = pred_bits(seed, s, r, PRED_SLOT_POISSON, t);
    const float U = u01_open(b.v[0]) - 0.5f, V = u01_open(b.v[1]);
    const float us = 0.5f - fabsf(U);               // >= 2^-25: u01_open never returns 0 or 1
    k = floorf((2.f * a_ / us + b_) * U + lam + 0.43f);
    if (k >= 0.f) kin = k;
    if (us >= 0.07f && V <= vr) break;
    if (k < 0.f || (us < 0.013f && V > us)) continue;
    if (logf(V * inv_alpha / (a_ / (us * us) + b_)) <= pred_poisson_logpmf(k, lam, loglam)) break;
  }
  return kin;
}

// the draw at (sample path s, global row r) from the member whose network output at that row is `loc` and whose
// aux row is (a0, a1, a2)
template <int OBS>
__device__ __forceinline__ float predictive_draw(uint64_t seed, uint32_t s, uint64_t r, float loc, float a0, float a1,
                                                 float a2) {
#pragma clang fp contract(off)
  if constexpr (OBS == BNF_OBS_NORMAL) {
    const Philox b = pred_bits(seed, s, r, PRED_SLOT_BASE, 0);
    return loc + a0 * std_normal(b.v[0], b.v[1]);
  }
  if constexpr (OBS == BNF_OBS_ZINB) {
    if (a2 != a2) return a2;                       // a NaN inflation probability fails the compare: it would never inflate
    const Philox b = pred_bits(seed, s, r, PRED_SLOT_BASE, 0);
    if (u01_open(b.v[2]) < a2) return (loc != loc || a1 != a1) ? loc + a1 : 0.f;   // NaN parameters: a NaN, not the 0
  }
  const float logits = -logf(a1) - logf(softplusf(loc));
  const float lrate = pred_log_gamma(seed, s, r, 1.f / a1) + logits;
  return pred_poisson(seed, s, r, expf(lrate));
}

// out (S, R) f32: sample paths sample0 .. sample0 + S of the rows row0 .. row0 + R (loc holds those R columns).
// Adjacent lanes take adjacent rows of one sample: one coalesced 4-byte store per draw.  grid (ceil(R / 1024), <= S):
// a thread takes 4 rows 256 apart and strides over the samples, so the component draw is shared by 4 row draws.
template <int OBS>
__global__ __launch_bounds__(256) void k_predictive_samples(const float* __restrict__ loc, const float* __restrict__ aux,
                                                            int32_t M, int64_t R, int64_t S, uint64_t seed, int64_t row0,
                                                            int64_t sample0, const double* __restrict__ cum,
                                                            float* __restrict__ out) {
  const int64_t base = (int64_t)blockIdx.x * (256 * kPredRowsPerThread) + threadIdx.x;
  for (int64_t s = blockIdx.y; s < S; s += gridDim.y) {
    const uint32_t sg = (uint32_t)(sample0 + s);
    const int32_t c = pred_component(seed, sg, M, cum);
    const float a0 = aux[c * 3], a1 = aux[c * 3 + 1], a2 = aux[c * 3 + 2];
    const float* lrow = loc + (int64_t)c * R;
    float* orow = out + s * R;
#pragma unroll 1
    for (int i = 0; i < kPredRowsPerThread; ++i) {
      const int64_t j = base + i * 256;
      if (j < R) orow[j] = predictive_draw<OBS>(seed, sg, (uint64_t)(row0 + j), lrow[j], a0, a1, a2);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Group totals of the sample paths, out (S, G) f64, without materialising the S x R draws.  The rows arrive sorted by
// group as CSR: group g owns the positions [seg_offsets[g], seg_offsets[g + 1]) of seg_rows.  Deterministic: no
// floating-point atomics, and the order of every sum depends only on the grouping.
//   The POSITION axis is cut into tiles of kPredTile = 1024, whatever the groups are: one huge group fills the device
//   (R / 1024 blocks per sample stride), a million tiny groups share blocks (up to 1024 per block).
//   pass 1 (this kernel, block = tile, strided over the samples): draws the tile's values -- the floats the per-row kernel
//     would store -- and sums, in f64, every piece (group x tile).  A tile inside one group: fixed tree (4 per thread,
//     wave butterfly, 4 waves).  A mixed tile: segmented Hillis-Steele scan in LDS, as many steps as the longest piece
//     needs (none for singletons).  A group that lies inside the tile goes to out directly; a piece of a group that
//     crosses a tile edge goes to the tile's slot 0 (the group holds the tile's first position) or slot 1
//     (partial: (S, tiles, 2) f64).
//   pass 2 (k_predictive_group_combine): one wave per (first tile of a crossing group, sample) adds that group's pieces
//     in tile order (lane = tile mod 64, then the butterfly).
// The group of a position is found by bisection of seg_offsets once per block, not per sample.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int32_t pred_group_of(const int32_t* __restrict__ seg_offsets, int32_t G, int64_t p) {
  int32_t lo = 0, hi = G;                                // seg_offsets[lo] <= p < seg_offsets[hi]
  while (hi - lo > 1) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if ((int64_t)seg_offsets[mid] <= p) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

enum : int { PRED_DEST_NONE = 0, PRED_DEST_OUT = 1, PRED_DEST_SLOT0 = 2, PRED_DEST_SLOT1 = 3 };

__device__ __forceinline__ void pred_store_piece(int kind, int32_t g, double v, int64_t s, int32_t G, int64_t tile,
                                                 int64_t n_tiles, double* __restrict__ partial,
                                                 double* __restrict__ out) {
  if (kind == PRED_DEST_OUT) out[s * G + g] = v;
  else if (kind != PRED_DEST_NONE) partial[(s * n_tiles + tile) * 2 + (kind - PRED_DEST_SLOT0)] = v;
}

template <int OBS>
__global__ __launch_bounds__(256) void k_predictive_group_sums(
    const float* __restrict__ loc, const float* __restrict__ aux, int32_t M, int64_t R,
    const int32_t* __restrict__ seg_offsets, const int32_t* __restrict__ seg_rows, int32_t G, int64_t S, uint64_t seed,
    int64_t row0, int64_t sample0, const double* __restrict__ cum, double* __restrict__ partial,
    double* __restrict__ out) {
  __shared__ double xs[2][kPredTile];
  __shared__ double wsum[2][4];
  __shared__ int s_maxlen, s_kind, s_g;
  const int tid = threadIdx.x;
  const int64_t tile = blockIdx.x, n_tiles = gridDim.x;
  const int64_t tile0 = tile * kPredTile;
  const int64_t tile_end = tile0 + kPredTile < R ? tile0 + kPredTile : R;
  const int n_valid = (int)(tile_end - tile0);

  int32_t row[kPredRowsPerThread], ps[kPredRowsPerThread], grp[kPredRowsPerThread];
  int kind[kPredRowsPerThread];
  if (tid == 0) s_maxlen = 0;
  __syncthreads();
  int maxlen = 0;
#pragma unroll
  for (int i = 0; i < kPredRowsPerThread; ++i) {
    const int q = i * 256 + tid;
    row[i] = -1; ps[i] = q; grp[i] = 0; kind[i] = PRED_DEST_NONE;
    if (q < n_valid) {
      const int64_t p = tile0 + q;
      const int32_t g = pred_group_of(seg_offsets, G, p);
      const int64_t o0 = seg_offsets[g], o1 = seg_offsets[g + 1];
      const int32_t rr = seg_rows[p];
      row[i] = (rr >= 0 && (int64_t)rr < R) ? rr : -1;       // a row outside the table adds nothing
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
      v[i] = row[i] >= 0 ? (double)predictive_draw<OBS>(seed, sg, (uint64_t)(row0 + row[i]), lrow[row[i]], a0, a1, a2) : 0.0;
    if (one_piece) {
      const double t = wave_sum_f64(((v[0] + v[1]) + v[2]) + v[3]);
      if ((tid & 63) == 0) wsum[it & 1][tid >> 6] = t;
      __syncthreads();
      if (tid == 0)
        pred_store_piece(u_kind, u_g, ((wsum[it & 1][0] + wsum[it & 1][1]) + wsum[it & 1][2]) + wsum[it & 1][3], s, G, tile,
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
      for (int i = 0; i < kPredRowsPerThread; ++i) pred_store_piece(kind[i], grp[i], v[i], s, G, tile, n_tiles, partial, out);
    }
  }
}

// pass 2: block = 4 waves, wave = (tile blockIdx.x, sample blockIdx.y * 4 + wave).  Only the wave of a tile in which a
// group STARTS and which that group leaves through the far edge has work: it owns that group's total.
__global__ __launch_bounds__(256) void k_predictive_group_combine(const int32_t* __restrict__ seg_offsets, int32_t G,
                                                                  int64_t R, int64_t S,
                                                                  const double* __restrict__ partial,
                                                                  double* __restrict__ out) {
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
  double acc = 0.0;
  for (int64_t j = tile + lane; j <= last && j < n_tiles; j += 64)
    acc += partial[(s * n_tiles + j) * 2 + ((j == tile && o0 != tile0) ? 1 : 0)];
  acc = wave_sum_f64(acc);
  if (lane == 0) out[s * G + g] = acc;
}

}  // namespace bnf
