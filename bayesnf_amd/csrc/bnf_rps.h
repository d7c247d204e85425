// bnf_rps.h -- the ranked probability score of NB / ZINB forecasts on the device (bnf_count_rps): the CRPS of a count
// forecast, which bnf_predictive_scores has for the NORMAL observation model only.  Inputs are what bnf_forward writes
// (loc (M, R), aux (M, 3)) and the observations y (R,); the per-member laws are those of bnf_sampling.h / bnf_scoring.h:
//       NB      total_count tc = 1 / aux[1], logits = -log aux[1] - log softplus(loc): with sm = aux[1] softplus(loc),
//               q = 1 / (1 + sm):  pmf(k + 1) = pmf(k) q (k + tc) / (k + 1),  cdf(k) = I_{1 - q}(tc, k + 1)
//       ZINB    F = aux[2] + (1 - aux[2]) F_NB
//   rps_r = sum_{k >= 0} (F_r(k) - 1{k >= y_r})^2,   F_r = (1 / M) sum_m F_{m,r}
// A row whose y is NaN, infinite, negative or not an integer gives NaN.
//
// The window.  The infinite sum is evaluated term by term on [a_r, b_r) and in closed form outside, eps = 1e-9:
//   per member, anchor k* = floor(mean): pmf(k*) from lgamma in f64, cdf(k*) from one betainc_xc call; then the pmf
//     recurrence downwards, a_m = the smallest k with cdf(k - 1) < eps (0 if there is none): below a_m the member's NB part
//     is below eps and is taken as 0;
//   a_r = min_m a_m.  Below a_r every term is P0^2 (k < y) or (1 - P0)^2 (k >= y), P0 = mean_m aux[m][2] (NB: 0);
//   from a_r upwards tiles of 64 consecutive k are summed until, at the end of a tile, every member is past its mean and
//     its upper tail is below eps by the geometric bound  sum_{j >= k} pmf(j) <= pmf(k) / (1 - r), r = max(q, pmf(k + 1) /
//     pmf(k))  (the ratio falls with k for tc >= 1 and rises towards q for tc < 1).  b_r = the end of that tile: a whole
//     number of tiles from a_r, and the terms up to it are summed, not approximated.  (1 - cdf < eps is NOT the test: the
//     anchor's pmf carries the relative error of lgamma, 1e-9 at a mean of 1e6, and with it the summed mass.)
//   at and above b_r every term is 1 (k < y) or 0 (k >= y).
//   Truncation, term by term (t(k) = 1 - F(k) the mixture's upper tail, l(k) = F(k) - P0 its NB part, both < eps outside):
//     k < a_r, k < y:   F^2 for P0^2, off by < 2 eps + eps^2         -- min(a_r, y) terms
//     k < a_r, k >= y:  (1 - F)^2 for (1 - P0)^2, off by < 2 eps     -- (a_r - y)^+ terms
//     k >= b_r, k < y:  F^2 for 1, off by 1 - F^2 <= 2 t(k) < 2 eps  -- (y - b_r)^+ terms
//     k >= b_r, k >= y: t(k)^2 for 0.  Past b_r every member's pmf falls at least geometrically with its ratio r < 1, hence
//                       so does its tail: t(k) <= eps r^(k - b_r), and the sum of t(k)^2 is <= eps^2 / (1 - r^2) <= eps^2 / (1 - r)
//                       with r the largest ratio among the members.
//   Each closed-form term is off by at most ~2 eps of a value that is itself of order one: the error is about 2e-9 of the
//   closed-form part of the score, plus eps^2 / (1 - r) -- far under the f32 result.
// The cap.  b_r - a_r > BNF_RPS_MAX_TERMS, or a member whose anchor lies more than BNF_RPS_MAX_TERMS above its a_m: the
//   row gives NaN (after at most that many steps: the work per row is bounded).  The grid's far corner (mean 1e6,
//   total_count 0.05) would need 3e8 terms; a strided or quadrature form for such rows is out of scope here.
//   A member whose parameters are not finite, or whose mean is 0 or beyond 2^52, gives NaN as well.
//
// Member weights (bnf_count_rps_weighted, WEIGHTED below): F_r = sum_m w_m F_{m,r} and P0 = sum_m w_m aux[m][2], w on
//   the simplex.  Window, eps and cap are the same, and so is the truncation argument: outside [a_r, b_r) every member's
//   tail is below eps, and a weighted mean of tails that are each below eps is below eps; past b_r it still falls with the
//   largest ratio among the members.  The weights are not read by the library's host side: weights off the simplex give a
//   meaningless score, never an access outside loc / aux / wts.  A member of weight exactly 0 adds nothing to F but still
//   widens the window (and can cap the row), and a NaN in its parameters still gives NaN: the Python layer drops such
//   members before the call.  w_m multiplies F_{m,r}(k) where lane j adds the members of one k, in member order.
//
// Arithmetic: softplus in f32 (as count_mix_cdf), everything after it f64.  Every sum is in an order the shapes fix (members
// in order inside a tile column, member chunks in order, k over lanes then the wave butterfly): no floating-point atomics,
// two calls give the same bits.
//
// k_count_rps: one wave per row (rows differ in cost by 1e4: the dispatcher balances them), members in lanes, k sequential.
//   A lane carries its member's (pmf, cdf) through a tile of 64 k (2 dependent f64 operations per k; 1 / (k + 1) is the
//   same for every member: lane j forms it once per tile, the members read it as an LDS broadcast) and writes
//   aux[2] + (1 - aux[2]) cdf to tile[k][member] (pitch 65 doubles: the write is contiguous, the transposed read below hits
//   64 different banks); then the lanes change role: lane j adds the members of k = k0 + j in member order -- one LDS read
//   and one add per (k, member) where a cross-lane f64 butterfly per k would cost ~18.  More than 64 members: chunks of 64
//   one after the other into the same tile, their state (q, tc - 1, pmf, cdf, a_m, k*) in LDS, 48 bytes per member, read and
//   written once per tile -- hence BNF_RPS_MAX_MEMBERS.  Every LDS byte read has been written by this kernel: the tile
//   columns of a short last chunk are neither written nor read.
#pragma once

#include "bnf_sampling.h"
#include "bnf_scoring.h"

namespace bnf {

constexpr int kRpsTile = 64;                       // consecutive k per tile = lanes of the wave
constexpr int kRpsPitch = kRpsTile + 1;            // doubles per tile row
constexpr int kRpsState = 6;                       // doubles of state per member
constexpr double kRpsEps = 1e-9;
constexpr int64_t kRpsMaxTerms = BNF_RPS_MAX_TERMS;
static_assert(kRpsMaxTerms % kRpsTile == 0, "the cap is a whole number of tiles");

constexpr size_t rps_lds_bytes(int64_t M) {
  return sizeof(double) * (size_t)(kRpsTile * kRpsPitch + kRpsTile + kRpsState * (((M + 63) / 64) * 64));
}
static_assert(rps_lds_bytes(BNF_RPS_MAX_MEMBERS) <= 160 * 1024, "LDS per workgroup");

__device__ __forceinline__ double wave_min_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
  return v;
}

template <int OBS, bool WEIGHTED>
__global__ __launch_bounds__(64) __attribute__((flatten)) void k_count_rps(const float* __restrict__ loc,
                                                                           const float* __restrict__ aux,
                                                                           const double* __restrict__ wts, int32_t M, int64_t R,
                                                                           const float* __restrict__ y,
                                                                           float* __restrict__ rps) {
  extern __shared__ __attribute__((aligned(16))) double rps_sm[];
  const int lane = threadIdx.x;
  const int32_t n_chunks = (M + 63) >> 6;
  const int32_t Mp = n_chunks << 6;
  double* tile = rps_sm;                              // [k - k0][member of the chunk], pitch kRpsPitch
  double* rk = tile + kRpsTile * kRpsPitch;           // 1 / (k0 + j + 1)
  double* sq = rk + kRpsTile;                         // per member: q, tc - 1, pmf, cdf, a_m, k*
  double* stc = sq + Mp;
  double* spm = stc + Mp;
  double* scd = spm + Mp;
  double* sa = scd + Mp;
  double* sks = sa + Mp;
  const float nanf_ = __builtin_nanf("");

  double p0 = 0.0;                                    // mean zero inflation: the same for every row and lane -- M <= 2,048
                                                      // cached loads per block, members in order (as the restatement adds them)
  if constexpr (OBS == BNF_OBS_ZINB) {
    if constexpr (WEIGHTED) {
      for (int32_t m = 0; m < M; ++m) p0 += wts[m] * (double)aux[m * 3 + 2];
    } else {
      for (int32_t m = 0; m < M; ++m) p0 += (double)aux[m * 3 + 2];
      p0 /= (double)M;
    }
  }

  for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {
    const float yv = y[r];
    if (!(score_finite(yv) && yv >= 0.f && yv == floorf(yv))) {          // the same in every lane
      if (lane == 0) rps[r] = nanf_;
      continue;
    }
    __syncthreads();                                   // the previous row's reads are done

    // ---- anchor at the mean, walk down to a_m --------------------------------------------------------------------
    double a_min = INFINITY;
    bool bad = false;
    for (int32_t c = 0; c < n_chunks; ++c) {
      const int32_t m = c * 64 + lane;
      if (m < M) {
        const double s = (double)aux[m * 3 + 1];
        const double sm = s * (double)softplusf(loc[(int64_t)m * R + r]);
        const double tc = 1.0 / s;
        const double q = 1.0 / (1.0 + sm);
        const double mu = tc / sm;
        double k = floor(mu);
        double pm = exp(lgamma(k + tc) - lgamma(k + 1.0) - lgamma(tc) - tc * log1p(1.0 / sm) - k * log1p(sm));
        double cd = betainc_xc(tc, 1.0 + k, sm / (1.0 + sm), q);
        bad = bad || !(sm > 0.0 && mu < 4503599627370496.0 && pm > 0.0 && pm < INFINITY && cd == cd);
        const double iq = 1.0 / q;
        int32_t steps = 0;
#pragma unroll 1
        while (k > 0.0 && cd - pm >= kRpsEps && steps < kRpsMaxTerms) {
          cd -= pm;
          pm = pm * k * iq / (k - 1.0 + tc);
          k -= 1.0;
          ++steps;
        }
        bad = bad || (k > 0.0 && cd - pm >= kRpsEps);                     // the walk hit the cap
        sq[m] = q; stc[m] = tc - 1.0; spm[m] = pm; scd[m] = cd; sa[m] = k; sks[m] = floor(mu);
        a_min = fmin(a_min, k);
      }
    }
    if (__ballot(bad) != 0ull) {                       // the same in every lane
      if (lane == 0) rps[r] = nanf_;
      continue;
    }
    const double a_r = wave_min_f64(a_min);

    // ---- tiles of 64 k from a_r --------------------------------------------------------------------------------------
    const double yd = (double)yv, dM = (double)M;
    double total = 0.0, k0 = a_r;
    int64_t span = 0;
    bool all_done;
    do {
      __syncthreads();                                 // the previous tile's reads of rk are done
      rk[lane] = 1.0 / (k0 + (double)lane + 1.0);
      __syncthreads();
      double acc = 0.0;
      bool done = true;
      const double kn = k0 + (double)kRpsTile;
      for (int32_t c = 0; c < n_chunks; ++c) {
        const int32_t m = c * 64 + lane;
        const int32_t n = M - c * 64 < 64 ? M - c * 64 : 64;
        if (m < M) {
          const double q = sq[m], tcm1 = stc[m], a = sa[m];
          double pm = spm[m], cd = scd[m];
          double pi = 0.0, w = 1.0;
          if constexpr (OBS == BNF_OBS_ZINB) { pi = (double)aux[m * 3 + 2]; w = 1.0 - pi; }
#pragma unroll 16
          for (int j = 0; j < kRpsTile; ++j) {
            const bool in = k0 + (double)j >= a;
            if constexpr (OBS == BNF_OBS_ZINB) tile[j * kRpsPitch + lane] = in ? pi + w * cd : pi;
            else tile[j * kRpsPitch + lane] = in ? cd : 0.0;
            const double pn = pm * (q * (1.0 + tcm1 * rk[j]));           // pmf(k + 1) = pmf(k) q (k + tc) / (k + 1)
            pm = in ? pn : pm;
            cd = in ? cd + pn : cd;
          }
          spm[m] = pm; scd[m] = cd;
          const double rr = fmax(q, q * (1.0 + tcm1 / (kn + 1.0)));
          done = done && kn > sks[m] && kn > a && pm < kRpsEps * (1.0 - rr);
        }
        __syncthreads();
#pragma unroll 8
        for (int32_t i = 0; i < n; ++i) {
          if constexpr (WEIGHTED) acc += wts[c * 64 + i] * tile[lane * kRpsPitch + i];
          else acc += tile[lane * kRpsPitch + i];
        }
        __syncthreads();                               // the next chunk overwrites the tile
      }
      const double d = (WEIGHTED ? acc : acc / dM) - (k0 + (double)lane >= yd ? 1.0 : 0.0);
      total += d * d;
      all_done = __ballot(!done) == 0ull;
      k0 = kn;
      span += kRpsTile;
    } while (!all_done && span < kRpsMaxTerms);
    total = wave_sum_f64(total);
    if (lane == 0) {
      const double n_lt = fmin(yd, a_r), n_ge = a_r - n_lt;
      const double v = p0 * p0 * n_lt + (1.0 - p0) * (1.0 - p0) * n_ge + total + fmax(yd - k0, 0.0);
      rps[r] = all_done ? (float)v : nanf_;
    }
  }
}

}  // namespace bnf
