// bnf_scoring.h -- held-out observations scored against the ensemble on the device (bnf_predictive_scores): what a user
// of the reference computes on the host from `likelihood_model()` (log_prob, cdf) plus the mixture scores it has no call
// for.  Inputs are what bnf_forward writes (loc (M, R), aux (M, 3)) and the observations y (R,); the per-member laws
// are those of bnf_sampling.h:
//       NORMAL  N(loc, aux[0])
//       NB      total_count = 1 / aux[1], logits = -log aux[1] - log softplus(loc)
//       ZINB    the NB, replaced by 0 with probability aux[2]
//
//   member_ll (M,) f64   sum over the rows with a finite y of log p_m(y_r)
//   lpd (R,) f32         log((1 / M) sum_m p_m(y_r)), running max + scaled sum over the members
//   pit (2, R) f32       F(y_r) and F(y_r-) of the equal-weight mixture
//   crps (R,) f32        NORMAL: (1 / M) sum_i A(y - mu_i, s_i) - (1 / (2 M^2)) sum_ij A(mu_i - mu_j, sqrt(s_i^2 + s_j^2)),
//                        A(m, s) = m (2 Phi(m / s) - 1) + 2 s phi(m / s)                       (Grimit et al. 2006)
// A row whose y is not finite gives NaN in every per-row output and adds nothing to member_ll.
// bnf_predictive_scores_weighted (WEIGHTED below), w (M,) f64 on the simplex, the forecast sum_m w_m p_m:
//   lpd   log sum_m w_m p_m(y_r);   pit   sum_m w_m F_m on either side of y_r
//   crps  sum_i w_i A(y - mu_i, s_i) - [sum_{j<i} w_i w_j A(mu_i - mu_j, sqrt(s_i^2 + s_j^2)) + sum_i w_i^2 s_i / sqrt(pi)]
//   Each f32 term is converted to double and multiplied by w_m there.  The weights are not validated (reading them would
//   cost a sync): weights off the simplex give meaningless numbers, never an access outside loc / aux / wts.
//
// Arithmetic: every per-(member, row) term is f32 (the NORMAL log density: formed in f64 from the f32 difference y - loc
// and rounded to f32 once); every sum over members, over member pairs and over rows is f64, in an
// order that depends on the shapes alone (no floating-point atomics): two calls give the same bits.
//   k_score_member_ll + k_score_member_ll_combine   rows cut into tiles of kScoreTile: fixed tree per (member, tile)
//     (4 per thread, wave butterfly, 4 waves), then one wave per member adds the tiles (lane = tile mod 64, butterfly).
//   k_score_crps_pairs                              the pair sum, see there.
//   k_score_rows                                    one lane per row, members in order; finishes the CRPS.
//   k_score_count_pit                               NB / ZINB: the mixture CDF on either side of y.
#pragma once

#include "bnf_quantiles.h"
#include "bnf_sampling.h"

namespace bnf {

constexpr int kScoreTile = BNF_SCORE_ROW_TILE;       // rows per block of the member_ll and pair kernels
constexpr int kScoreRowsPerThread = 4;
constexpr int kScoreChunk = BNF_SCORE_MEMBER_CHUNK;  // members i whose mu_i a thread of the pair kernel holds in registers
constexpr int kScoreMaxSlots = BNF_SCORE_MAX_SLOTS;  // partial pair sums per row
static_assert(kScoreTile == 256 * kScoreRowsPerThread, "row tile = one block of 256 threads x 4 rows");

// log p_m(y) of one member at one row.  The count forms are row_loss_eval's (bnf_device.h, where the reasons are written
// down): terms of the size of the result -- lgamma recurrence below y = 10, Stirling's series with the y log y terms taken
// out by hand from there on, log1p forms of log p and log(1 - p) -- so that held-out and training likelihood agree.
// shape = aux[1] and pi = aux[2] arrive transformed (bnf_forward), where row_loss_eval starts from the raw parameters.
template <int OBS>
__device__ __forceinline__ float score_log_density(float yv, float loc, float a0, float a1, float a2) {
  if constexpr (OBS == BNF_OBS_NORMAL) {
    // f64 from the f32 difference, rounded once: at |z| = 10 the f32 chain (z, z^2, the two subtractions) is off by 1e-5
    // of a value the rows of member_ll then sum to a few units (sigma = 0.01, members three sigma apart)
    const double z = (double)(yv - loc) / (double)a0;
    return (float)(-0.5 * z * z - log((double)a0) - 0.918938533204672742);
  } else {
    const float shape = a1;
    const float tc = 1.0f / shape;
    const float mean = softplusf(loc);
    const float sm = shape * mean;              // e^-logits
    const float rsm = 1.0f / sm;                // e^logits
    const float mu = tc * rsm;                  // the NB mean
    const float lsn = -log1pf(rsm);             // log sigmoid(-logits)
    const float n = tc + yv, den = tc + mu, delta = yv - mu;
    float lp;
    if (yv >= 10.f) {
      const float l1 = fabsf(delta) <= 0.5f * den ? log1pf(delta / den) : logf(n / den);
      const float x2 = tc * (mu - yv) / (yv * den);
      const float l2 = fabsf(x2) <= 0.5f ? log1pf(x2) : logf((n / den) * (mu / yv));
      const float a_tc = tc >= 10.f ? 0.5f * logf(tc) - 0.918938533204672742f - stirling_corr(tc)
                                    : tc * logf(tc) - tc - lgammaf(tc);
      lp = tc * l1 + yv * l2 - 0.5f * (logf(n) + logf(yv)) + a_tc + stirling_corr(n) - stirling_corr(yv);
    } else if (yv == floorf(yv)) {
      const float sgp = 1.0f / (1.0f + sm);     // sigmoid(logits)
      float acc = 0.f;
#pragma unroll 1
      for (float j = 0.f; j < yv; j += 1.0f) acc += logf((tc + j) / (1.0f + j) * sgp);
      lp = tc * lsn + acc;
    } else {
      lp = tc * lsn - yv * log1pf(sm) + lgammaf(n) - lgammaf(1.0f + yv) - lgammaf(tc);
    }
    if constexpr (OBS == BNF_OBS_ZINB) {
      if (yv == 0.f) lp = logf((1.0f - a2) * expf(lp) + a2);
      else lp += log1pf(-a2);
    }
    return lp;
  }
}

__device__ __forceinline__ bool score_finite(float v) { return fabsf(v) <= 3.4028234664e38f; }   // false for NaN

// A(d, s) = d erf(d / (s sqrt 2)) + s sqrt(2 / pi) exp(-d^2 / (2 s^2)) with c1 = 1 / (s sqrt 2), c2 = s sqrt(2 / pi)
__device__ __forceinline__ float score_abs_moment(float d, float c1, float c2) {
  const float t = d * c1;
  return d * erff(t) + c2 * expf(-t * t);
}

// ---------------------------------------------------------------------------------------------------------------------
// member_ll.  partial (M, n_tiles) f64; grid (n_tiles, <= M): a block owns one tile of kScoreTile rows and strides over
// the members.
// ---------------------------------------------------------------------------------------------------------------------
template <int OBS>
__global__ __launch_bounds__(256) void k_score_member_ll(const float* __restrict__ loc, const float* __restrict__ aux,
                                                         int32_t M, int64_t R, const float* __restrict__ y,
                                                         double* __restrict__ partial) {
  __shared__ double wsum[4];
  const int tid = threadIdx.x;
  const int64_t n_tiles = gridDim.x;
  const int64_t base = (int64_t)blockIdx.x * kScoreTile + tid;
  float yv[kScoreRowsPerThread];
  bool ok[kScoreRowsPerThread];
#pragma unroll
  for (int i = 0; i < kScoreRowsPerThread; ++i) {
    const int64_t r = base + i * 256;
    yv[i] = r < R ? y[r] : 0.f;
    ok[i] = r < R && score_finite(yv[i]);
  }
  for (int32_t m = blockIdx.y; m < M; m += gridDim.y) {
    const float a0 = aux[m * 3], a1 = aux[m * 3 + 1], a2 = aux[m * 3 + 2];
    const float* lrow = loc + (int64_t)m * R;
    double v[kScoreRowsPerThread];
#pragma unroll 1
    for (int i = 0; i < kScoreRowsPerThread; ++i)
      v[i] = ok[i] ? (double)score_log_density<OBS>(yv[i], lrow[base + i * 256], a0, a1, a2) : 0.0;
    const double t = wave_sum_f64(((v[0] + v[1]) + v[2]) + v[3]);
    if ((tid & 63) == 0) wsum[tid >> 6] = t;
    __syncthreads();
    if (tid == 0) partial[(int64_t)m * n_tiles + blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    __syncthreads();                                         // the next member overwrites wsum
  }
}

// one wave per member adds its tiles in tile order
__global__ __launch_bounds__(256) void k_score_member_ll_combine(const double* __restrict__ partial, int32_t M,
                                                                 int64_t n_tiles, double* __restrict__ member_ll) {
  const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const int lane = threadIdx.x & 63;
  double acc = 0.0;
  for (int64_t j = lane; j < n_tiles; j += 64) acc += partial[m * n_tiles + j];
  acc = wave_sum_f64(acc);
  if (lane == 0) member_ll[m] = acc;
}

// ---------------------------------------------------------------------------------------------------------------------
// The CRPS pair sum: P_r = sum over j < i of A(mu_i[r] - mu_j[r], sqrt(s_i^2 + s_j^2)), M (M - 1) / 2 evaluations of erf
// and exp per row -- 1.8 M per row for a VI fit of 1,920 components.  (The diagonal, A(0, s) = 2 s phi(0), does not depend
// on the row: k_score_rows adds it.)
//   lanes are rows: loc[m * R + r] is a coalesced 4-byte load per lane, a thread owns 4 rows 256 apart;
//   the members i are cut into chunks of kScoreChunk = 8: a thread holds the 8 x 4 values mu_i of a chunk in registers and
//     streams mu_j, j < i, past them (the next j is loaded while this one is evaluated): 4 loads per 32 evaluations;
//   s_i^2 + s_j^2 -> 1 / (s sqrt 2) and s sqrt(2 / pi) are the same in every lane; they are formed once per pair and
//     thread and serve its 4 rows (gfx950 has no scalar float unit to move them to: a uniform vector instruction costs
//     what a divergent one does, so the 4 rows per thread are what amortises them, ~2 of ~40 instructions per evaluation);
//   chunk c costs ~ c, so chunks are dealt out in pairs (q, n_chunks - 1 - q) -- every slot the same work -- and the
//     slots round-robin over gridDim.y <= kScoreMaxSlots blocks per row tile;
//   every term is added to the row's f64 sum as it is formed (v_cvt + v_add_f64, 2 of ~40): a plain f32 sum of 1.8 M
//     terms would lose 1e-4.
// partial (gridDim.y, R) f64: block (x, p) writes the sum of its slots' pairs for the rows of tile x, always.
// Bound by the VALU: erff + expf + the rest are ~40 vector instructions per evaluation against 4 bytes loaded per 8.
// ---------------------------------------------------------------------------------------------------------------------
// WEIGHTED (bnf_predictive_scores_weighted): the sum of w_i w_j A(...).  wts (M,) f64 is read at the indices aux is read
// at; w_i w_j is the same in every lane and is formed once per pair next to c1, c2 (one v_mul_f64 per evaluation more).
template <bool FULL, bool WEIGHTED>
__device__ __forceinline__ void score_pairs_chunk(const float* __restrict__ loc, const float* __restrict__ aux,
                                                  const double* __restrict__ wts, int64_t R,
                                                  const int64_t (&row)[kScoreRowsPerThread], int32_t i0, int32_t ni,
                                                  double (&acc)[kScoreRowsPerThread]) {
  float mui[kScoreChunk][kScoreRowsPerThread], vi[kScoreChunk];
  double wi[WEIGHTED ? kScoreChunk : 1];
#pragma unroll
  for (int ii = 0; ii < kScoreChunk; ++ii) {
    const int32_t i = (FULL || ii < ni) ? i0 + ii : i0;      // a short last chunk repeats its first member, unused
    const float s = aux[i * 3];
    vi[ii] = s * s;
    if constexpr (WEIGHTED) wi[ii] = wts[i];
#pragma unroll
    for (int k = 0; k < kScoreRowsPerThread; ++k) mui[ii][k] = loc[(int64_t)i * R + row[k]];
  }
  const int32_t j_end = i0 + ni - 1;                          // j < i <= i0 + ni - 1
  if (j_end <= 0) return;
  float muj[kScoreRowsPerThread];
#pragma unroll
  for (int k = 0; k < kScoreRowsPerThread; ++k) muj[k] = loc[row[k]];
#pragma unroll 1
  for (int32_t j = 0; j < j_end; ++j) {
    const float sj = aux[j * 3];
    const float vj = sj * sj;
    double wj = 0.0;
    if constexpr (WEIGHTED) wj = wts[j];
    float cur[kScoreRowsPerThread];
    const int32_t jn = j + 1 < j_end ? j + 1 : j;
#pragma unroll
    for (int k = 0; k < kScoreRowsPerThread; ++k) { cur[k] = muj[k]; muj[k] = loc[(int64_t)jn * R + row[k]]; }
#pragma unroll
    for (int ii = 0; ii < kScoreChunk; ++ii) {
      if (j < i0 ? (FULL || ii < ni) : (ii < ni && i0 + ii > j)) {      // the same in every lane
        const float s2 = vi[ii] + vj;
        const float rs = rsqrtf(s2);
        const float c1 = rs * 0.70710678118654752440f, c2 = (s2 * rs) * 0.79788456080286535588f;
        if constexpr (WEIGHTED) {
          const double ww = wi[ii] * wj;
#pragma unroll
          for (int k = 0; k < kScoreRowsPerThread; ++k) acc[k] += ww * (double)score_abs_moment(mui[ii][k] - cur[k], c1, c2);
        } else {
#pragma unroll
          for (int k = 0; k < kScoreRowsPerThread; ++k) acc[k] += (double)score_abs_moment(mui[ii][k] - cur[k], c1, c2);
        }
      }
    }
  }
}

template <bool WEIGHTED>
__global__ __launch_bounds__(256) void k_score_crps_pairs(const float* __restrict__ loc, const float* __restrict__ aux,
                                                          const double* __restrict__ wts, int32_t M, int64_t R,
                                                          double* __restrict__ partial) {
  const int64_t base = (int64_t)blockIdx.x * kScoreTile + threadIdx.x;
  int64_t row[kScoreRowsPerThread];
#pragma unroll
  for (int k = 0; k < kScoreRowsPerThread; ++k) row[k] = base + k * 256 < R ? base + k * 256 : R - 1;   // loads stay inside
  double acc[kScoreRowsPerThread] = {0.0, 0.0, 0.0, 0.0};
  const int32_t n_chunks = (M + kScoreChunk - 1) / kScoreChunk;
  const int32_t n_slots = (n_chunks + 1) / 2;
  for (int32_t q = blockIdx.y; q < n_slots; q += gridDim.y) {
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
      const int32_t c = half == 0 ? q : n_chunks - 1 - q;
      if (half == 1 && c == q) break;                         // an odd number of chunks: the middle one once
      const int32_t i0 = c * kScoreChunk;
      const int32_t ni = M - i0 < kScoreChunk ? M - i0 : kScoreChunk;
      if (ni == kScoreChunk) score_pairs_chunk<true, WEIGHTED>(loc, aux, wts, R, row, i0, ni, acc);
      else score_pairs_chunk<false, WEIGHTED>(loc, aux, wts, R, row, i0, ni, acc);
    }
  }
#pragma unroll
  for (int k = 0; k < kScoreRowsPerThread; ++k)
    if (base + k * 256 < R) partial[(int64_t)blockIdx.y * R + base + k * 256] = acc[k];
}

// ---------------------------------------------------------------------------------------------------------------------
// The per-row outputs: one lane per row, the members in order.  Any of lpd / pit / crps may be null.
//   lpd   running max mx and s = sum_m exp(lp_m - mx), s in f64 (1,920 f32 terms would cost 1e-5); finite as long as one
//         member's log density is -- also where every density underflows
//   pit   NORMAL: the mean of ndtrf, both rows (counts: k_score_count_pit)
//   crps  first term here, pair sum from k_score_crps_pairs' partials (added in slot order), diagonal sum_i s_i / sqrt(pi)
// WEIGHTED: every term of the three sums times w_m (the diagonal: w_m^2) in f64, and no division by M at the end:
//   lpd = mx + log sum_m w_m exp(lp_m - mx), pit = sum_m w_m Phi, crps = sum w A - (pairs + sum w^2 s / sqrt(pi)).
// ---------------------------------------------------------------------------------------------------------------------
template <int OBS, bool WEIGHTED>
__global__ __launch_bounds__(64) void k_score_rows(const float* __restrict__ loc, const float* __restrict__ aux,
                                                   const double* __restrict__ wts, int32_t M,
                                                   int64_t R, const float* __restrict__ y,
                                                   const double* __restrict__ pair_partial, int32_t n_partial,
                                                   float* __restrict__ lpd, float* __restrict__ pit,
                                                   float* __restrict__ crps) {
  const int64_t r = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (r >= R) return;
  const float yv = y[r];
  if (!score_finite(yv)) {
    const float nan = __builtin_nanf("");
    if (lpd) lpd[r] = nan;
    if (OBS == BNF_OBS_NORMAL && pit) { pit[r] = nan; pit[R + r] = nan; }
    if (crps) crps[r] = nan;
    return;
  }
  float mx = -INFINITY;
  double s = 0.0, cdf = 0.0, first = 0.0, diag = 0.0;
  const bool normal_sums = OBS == BNF_OBS_NORMAL && (pit || crps);
  if (lpd || normal_sums) {
#pragma unroll 1
    for (int32_t m = 0; m < M; ++m) {
      const float a0 = aux[m * 3], a1 = aux[m * 3 + 1], a2 = aux[m * 3 + 2];
      const float l = loc[(int64_t)m * R + r];
      double w = 1.0;
      if constexpr (WEIGHTED) w = wts[m];
      if (lpd) {
        const float lp = score_log_density<OBS>(yv, l, a0, a1, a2);
        const float nm = fmaxf(mx, lp);
        if (nm > -INFINITY) {
          if constexpr (WEIGHTED) s = s * (double)expf(mx - nm) + w * (double)expf(lp - nm);
          else s = s * (double)expf(mx - nm) + (double)expf(lp - nm);
          mx = nm;
        }
      }
      if constexpr (OBS == BNF_OBS_NORMAL) {
        if (normal_sums) {
          const float d = yv - l;
          const float cm = ndtrf(d / a0);
          const float am = score_abs_moment(d, 0.70710678118654752440f / a0, a0 * 0.79788456080286535588f);
          if constexpr (WEIGHTED) {
            cdf += w * (double)cm;
            first += w * (double)am;
            diag += (w * w) * (double)a0;
          } else {
            cdf += (double)cm;
            first += (double)am;
            diag += (double)a0;
          }
        }
      }
    }
  }
  if (lpd) lpd[r] = mx + logf((float)(WEIGHTED ? s : s / (double)M));
  if constexpr (OBS == BNF_OBS_NORMAL) {
    if (pit) {
      const float f = (float)(WEIGHTED ? cdf : cdf / (double)M);
      pit[r] = f;
      pit[R + r] = f;
    }
  }
  if constexpr (OBS == BNF_OBS_NORMAL) {
    if (crps) {
      double pairs = 0.0;
      for (int32_t p = 0; p < n_partial; ++p) pairs += pair_partial[(int64_t)p * R + r];
      const double dm = (double)M;
      if constexpr (WEIGHTED) crps[r] = (float)(first - (pairs + diag * 0.56418958354775628695));
      else crps[r] = (float)(first / dm - (pairs + diag * 0.56418958354775628695) / (dm * dm));
    }
  }
}

// pit of the count models: count_mix_cdf (bnf_quantiles.h, f64 for the reason given there) at floor(y) (blockIdx.y = 0) and
// at the largest integer below y (blockIdx.y = 1), 0 below the support.  One lane per (row, side).  `flatten`: left to
// itself hipcc calls count_mix_cdf as a function, and the call stack is 268 bytes of scratch per lane; inlined there is none.
template <bool WEIGHTED>
__global__ __launch_bounds__(64) __attribute__((flatten)) void k_score_count_pit(const float* __restrict__ loc, const float* __restrict__ aux,
                                                        const double* __restrict__ wts, int32_t M, int64_t R, int32_t obs, const float* __restrict__ y,
                                                        float* __restrict__ pit) {
  const int64_t r = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (r >= R) return;
  const float yv = y[r];
  float* out = pit + (int64_t)blockIdx.y * R;
  if (!score_finite(yv)) { out[r] = __builtin_nanf(""); return; }
  const float yf = floorf(yv);
  const float x = blockIdx.y == 0 ? yf : (yv == yf ? yf - 1.0f : yf);
  out[r] = x < 0.f ? 0.f : count_mix_cdf<WEIGHTED>(loc, aux, wts, M, R, obs, r, x);
}

}  // namespace bnf
