// bnf_quantiles.h -- mixture quantiles of the ensemble forecast: the Normal mixture's (exact by Chandrupatla's root
// finder, or moment-matched) and the NB / ZINB mixture's, with the cdf helpers the scores share: ndtrf, betainc_xc,
// count_mix_cdf.  Forecast unit only (bnf_forecast.hip): the non-template kernels in here have one host stub.
#pragma once

#include "bnf_device.h"
#include "../../include/bnf.h"

namespace bnf {

// ---------------------------------------------------------------------------
// mixture-of-Normals quantiles (inference.py:42-84)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_minmax_partial(const float* __restrict__ x, int64_t n,
                                                        float* __restrict__ part) {
  __shared__ float smin[4], smax[4];
  float lo = INFINITY, hi = -INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float v = x[i];
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
  lo = wave_min(lo);
  hi = wave_max(hi);
  if ((threadIdx.x & 63) == 0) {
    smin[threadIdx.x >> 6] = lo;
    smax[threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[blockIdx.x * 2] = fminf(fminf(smin[0], smin[1]), fminf(smin[2], smin[3]));
    part[blockIdx.x * 2 + 1] = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
  }
}

// bracket[0..1] = [min mu - 5 max sigma, max mu + 5 max sigma]
__global__ void k_bracket(const float* mean_part, int n_mean_part, const float* scale_part,
                          int n_scale_part, float* bracket) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float lo = INFINITY, hi = -INFINITY, smax = -INFINITY;
  for (int i = 0; i < n_mean_part; ++i) {
    lo = fminf(lo, mean_part[2 * i]);
    hi = fmaxf(hi, mean_part[2 * i + 1]);
  }
  for (int i = 0; i < n_scale_part; ++i) smax = fmaxf(smax, scale_part[2 * i + 1]);
  bracket[0] = lo - 5.f * smax;
  bracket[1] = hi + 5.f * smax;
}

__device__ __forceinline__ float ndtrf(float z) { return 0.5f * erfcf(-z * 0.70710678118654752440f); }

// Member weights (the *_weighted entry points): WEIGHTED is a template parameter of the kernels below and `wts`
// (n_members,) f64 is read only under it, so the unweighted instantiation is the arithmetic it was without it.  The
// weighted sums are f64: w_m times the f32 term, members in order.
template <bool WEIGHTED>
__device__ __forceinline__ float mix_cdf(const float* __restrict__ means,
                                         const float* __restrict__ scales, const double* __restrict__ wts,
                                         int64_t n_members, int64_t n_rows, int64_t r, float x) {
  if constexpr (WEIGHTED) {
    double acc = 0.0;
    for (int64_t m = 0; m < n_members; ++m) acc += wts[m] * (double)ndtrf((x - means[m * n_rows + r]) / scales[m]);
    return (float)acc;
  } else {
    float acc = 0.f;
    for (int64_t m = 0; m < n_members; ++m) acc += ndtrf((x - means[m * n_rows + r]) / scales[m]);
    return acc / (float)n_members;
  }
}

// Chandrupatla's bracketing root finder (the algorithm behind
// tfp.math.find_root_chandrupatla), one thread per row.
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void k_quantile_root(const float* __restrict__ means,
                                                       const float* __restrict__ scales,
                                                       const double* __restrict__ wts,
                                                       int64_t n_members, int64_t n_rows,
                                                       const float* __restrict__ bracket, float q,
                                                       float* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  const float vtol = 1e-5f, ptol = 1e-8f;
  float a = bracket[0], b = bracket[1];
  float fa = mix_cdf<WEIGHTED>(means, scales, wts, n_members, n_rows, r, a) - q;
  float fb = mix_cdf<WEIGHTED>(means, scales, wts, n_members, n_rows, r, b) - q;
  float c = a, fc = fa, t = 0.5f;
  float best = fabsf(fa) < fabsf(fb) ? a : b;
  float fbest = fabsf(fa) < fabsf(fb) ? fa : fb;
  for (int it = 0; it < 60 && fabsf(fbest) > vtol; ++it) {
    const float xn = a + t * (b - a);
    const float fn = mix_cdf<WEIGHTED>(means, scales, wts, n_members, n_rows, r, xn) - q;
    const bool same = (fn > 0.f) == (fa > 0.f) && (fn < 0.f) == (fa < 0.f);
    if (same) { c = a; fc = fa; }
    else { c = b; fc = fb; b = a; fb = fa; }
    a = xn; fa = fn;
    if (fabsf(fa) < fabsf(fb)) { best = a; fbest = fa; } else { best = b; fbest = fb; }
    const float tol = ptol / fabsf(b - c);
    if (tol > 0.5f || fbest == 0.f) break;
    const float xi = (a - b) / (c - b), phi = (fa - fb) / (fc - fb);
    if (phi * phi < xi && (1.f - phi) * (1.f - phi) < 1.f - xi) {
      t = (fa / (fb - fa)) * (fc / (fb - fc)) + ((c - a) / (b - a)) * (fa / (fc - fa)) * (fb / (fc - fb));
    } else {
      t = 0.5f;
    }
    t = fminf(fmaxf(t, tol), 1.f - tol);
    if (!(t == t)) t = 0.5f;
  }
  out[r] = best;
}

// moment-matched Normal quantile (inference.py:55-84)
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void k_quantile_approx(const float* __restrict__ means,
                                                         const float* __restrict__ scales,
                                                         const double* __restrict__ wts,
                                                         int64_t n_members, int64_t n_rows, float q,
                                                         float* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  // Two passes, f64, members in order: mean = sum w mu first, then var = sum w (sd^2 + (mu - mean)^2).  The one-pass
  // form sum w (sd^2 + mu^2) - mean^2 cancels at the data's own scale: mu = 1e5 with sd = 0.01 leaves sd^2 = 1e-4 out of
  // 1e10, nothing in f32 and 4 % off in f64.  Centred, an error e of the mean costs e^2 and every term is >= 0.
  double mean = 0.0;
  for (int64_t m = 0; m < n_members; ++m) {
    const double mu = means[m * n_rows + r];
    if constexpr (WEIGHTED) mean += wts[m] * mu;
    else mean += mu;
  }
  if constexpr (!WEIGHTED) mean /= (double)n_members;
  double var = 0.0;
  for (int64_t m = 0; m < n_members; ++m) {
    const double d = (double)means[m * n_rows + r] - mean, sd = scales[m];
    if constexpr (WEIGHTED) var += wts[m] * (sd * sd + d * d);
    else var += sd * sd + d * d;
  }
  if constexpr (!WEIGHTED) var /= (double)n_members;
  out[r] = (float)(mean + sqrt(var) * normcdfinv((double)q));
}

// ---------------------------------------------------------------------------
// count observation models: NB / ZINB forecast moments and mixture quantiles
// (inference.py:271-333, 497-502; TFP 0.24 NegativeBinomial / Mixture).
//   s = softplus(theta_shape) = aux[e][1], m = softplus(loc), tc = 1/s,
//   logits = -log s - log m  =>  e^logits = 1/(s m), sigmoid(-logits) = s m/(1+s m)
//   NB mean = tc e^logits = 1/(s^2 m), var = mean / sigmoid(-logits)
//   ZINB = Mixture([1-pi, pi], [NB, delta_0])
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_count_moments(const float* __restrict__ loc,
                                                       const float* __restrict__ aux,
                                                       int64_t n_members, int64_t n_rows, int32_t obs,
                                                       float* __restrict__ means,
                                                       float* __restrict__ part) {
  __shared__ float smean[4], ssd[4];
  float mx_mean = 0.f, mx_sd = 0.f;
  const int64_t n = n_members * n_rows;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = i / n_rows;
    const float s = aux[e * 3 + 1];
    const float m = softplusf(loc[i]);
    const float sm = s * m;
    float mean = 1.0f / (s * sm);
    float var = mean * (1.0f + sm) / sm;
    if (obs == BNF_OBS_ZINB) {
      const float pi = aux[e * 3 + 2];
      const float zmean = (1.0f - pi) * mean;
      var = (1.0f - pi) * (var + mean * mean) - zmean * zmean;
      mean = zmean;
    }
    means[i] = mean;
    mx_mean = fmaxf(mx_mean, mean);
    mx_sd = fmaxf(mx_sd, sqrtf(fmaxf(var, 0.f)));
  }
  mx_mean = wave_max(mx_mean);
  mx_sd = wave_max(mx_sd);
  if ((threadIdx.x & 63) == 0) { smean[threadIdx.x >> 6] = mx_mean; ssd[threadIdx.x >> 6] = mx_sd; }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[blockIdx.x * 2] = fmaxf(fmaxf(smean[0], smean[1]), fmaxf(smean[2], smean[3]));
    part[blockIdx.x * 2 + 1] = fmaxf(fmaxf(ssd[0], ssd[1]), fmaxf(ssd[2], ssd[3]));
  }
}

// bracket[2 + 0..1] = {max mean, max stddev}
__global__ void k_count_bracket(const float* part, int n_part, float* bracket) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float mm = 0.f, ms = 0.f;
  for (int i = 0; i < n_part; ++i) { mm = fmaxf(mm, part[2 * i]); ms = fmaxf(ms, part[2 * i + 1]); }
  bracket[2] = mm;
  bracket[3] = ms;
}

// continued fraction of the incomplete beta function (modified Lentz), f64: the
// prefactor a log x + b log(1-x) - lbeta(a,b) cancels catastrophically in f32 for the
// b ~ 1e3..1e5 the bracket reaches.
__device__ inline double beta_cf(double a, double b, double x) {
  const double tiny = 1e-300, eps = 1e-13;
  const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
  double c = 1.0, d = 1.0 - qab * x / qap;
  if (fabs(d) < tiny) d = tiny;
  d = 1.0 / d;
  double hh = d;
#pragma unroll 1
  for (int m = 1; m <= 2000; ++m) {
    const double m2 = 2.0 * m;
    double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
    d = 1.0 + aa * d; if (fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c; if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    hh *= d * c;
    aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
    d = 1.0 + aa * d; if (fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c; if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    const double del = d * c;
    hh *= del;
    if (fabs(del - 1.0) < eps) break;
  }
  return hh;
}

// regularised incomplete beta I_x(a, b) with xc = 1 - x supplied separately
__device__ inline double betainc_xc(double a, double b, double x, double xc) {
  if (x <= 0.0) return 0.0;
  if (xc <= 0.0) return 1.0;
  const double lnpre = lgamma(a + b) - lgamma(a) - lgamma(b) + a * log(x) + b * log(xc);
  if (x < (a + 1.0) / (a + b + 2.0)) return exp(lnpre) * beta_cf(a, b, x) / a;
  return 1.0 - exp(lnpre) * beta_cf(b, a, xc) / b;
}

// mean over members (WEIGHTED: sum of wts[e] times) of the (ZI)NB cdf at x >= 0, row r
template <bool WEIGHTED>
__device__ inline float count_mix_cdf(const float* __restrict__ loc, const float* __restrict__ aux,
                                      const double* __restrict__ wts, int64_t n_members, int64_t n_rows,
                                      int32_t obs, int64_t r, float x) {
  double acc = 0.0;
  for (int64_t e = 0; e < n_members; ++e) {
    const double s = aux[e * 3 + 1];
    const double sm = s * (double)softplusf(loc[e * n_rows + r]);
    double F = betainc_xc(1.0 / s, 1.0 + (double)x, sm / (1.0 + sm), 1.0 / (1.0 + sm));
    if (obs == BNF_OBS_ZINB) {
      const double pi = aux[e * 3 + 2];
      F = pi + (1.0 - pi) * F;
    }
    if constexpr (WEIGHTED) acc += wts[e] * F;
    else acc += F;
  }
  if constexpr (WEIGHTED) return (float)acc;
  else return (float)(acc / (double)n_members);
}

// one thread per row: Chandrupatla on [0, max mean + 1.1 rsqrt(1-q) max sd], then ceil;
// rows whose mixture pmf(0) already exceeds q are 0 (inference.py:319-333).
template <bool WEIGHTED>
__global__ __launch_bounds__(64) void k_count_quantile_root(const float* __restrict__ loc,
                                                            const float* __restrict__ aux,
                                                            const double* __restrict__ wts,
                                                            int64_t n_members, int64_t n_rows,
                                                            int32_t obs,
                                                            const float* __restrict__ bracket, float q,
                                                            float* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  const float vtol = 1e-5f, ptol = 1e-8f;
  float a = 0.f, b = bracket[2] + 1.1f * rsqrtf(1.0f - q) * bracket[3];
  float fa = count_mix_cdf<WEIGHTED>(loc, aux, wts, n_members, n_rows, obs, r, a) - q;
  if (fa > 0.f) { out[r] = 0.f; return; }
  float fb = count_mix_cdf<WEIGHTED>(loc, aux, wts, n_members, n_rows, obs, r, b) - q;
  float c = a, fc = fa, t = 0.5f;
  float best = fabsf(fa) < fabsf(fb) ? a : b;
  float fbest = fabsf(fa) < fabsf(fb) ? fa : fb;
  for (int it = 0; it < 60 && fabsf(fbest) > vtol; ++it) {
    const float xn = a + t * (b - a);
    const float fn = count_mix_cdf<WEIGHTED>(loc, aux, wts, n_members, n_rows, obs, r, xn) - q;
    const bool same = (fn > 0.f) == (fa > 0.f) && (fn < 0.f) == (fa < 0.f);
    if (same) { c = a; fc = fa; }
    else { c = b; fc = fb; b = a; fb = fa; }
    a = xn; fa = fn;
    if (fabsf(fa) < fabsf(fb)) { best = a; fbest = fa; } else { best = b; fbest = fb; }
    const float tol = ptol / fabsf(b - c);
    if (tol > 0.5f || fbest == 0.f) break;
    const float xi = (a - b) / (c - b), phi = (fa - fb) / (fc - fb);
    if (phi * phi < xi && (1.f - phi) * (1.f - phi) < 1.f - xi) {
      t = (fa / (fb - fa)) * (fc / (fb - fc)) + ((c - a) / (b - a)) * (fa / (fc - fa)) * (fb / (fc - fb));
    } else {
      t = 0.5f;
    }
    t = fminf(fmaxf(t, tol), 1.f - tol);
    if (!(t == t)) t = 0.5f;
  }
  out[r] = ceilf(best);
}

}  // namespace bnf
