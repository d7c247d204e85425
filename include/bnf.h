/* bnf.h -- C ABI of the MI355X-native BayesNF ensemble engine (libbnf_hip.so).
 *
 * The reference (google/bayesnf, /root/reference) has no FFI: its hot path is
 * reached through three Python calls (src/bayesnf/spatiotemporal.py:400,529,634
 * -> src/bayesnf/inference.py fit_map:376 / fit_vi:336 / predict_bnf:461) that
 * trace into one XLA program (`jax.pmap(jax.vmap(...))`, inference.py:577-619,
 * :727-745, :474-477).  This header is the boundary a maintainer would bind in
 * place of that XLA program (ctypes stub in INTEGRATION.md); each entry point
 * cites the reference code it replaces.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - every pointer marked DEVICE is HBM memory owned by the caller (the Python
 *     side uses torch-ROCm tensors purely as containers); the library owns only
 *     the opaque handle and a few HIP events.
 *   - all work is enqueued on the caller's HIP stream (`stream`, a hipStream_t
 *     passed as void*; NULL = the default stream).  Nothing synchronises unless
 *     stated.
 *   - return value 0 = ok, negative = error; bnf_last_error() returns a
 *     thread-local message.  Nothing throws across the ABI.
 *   - one handle per GPU, used from one host thread at a time.
 *   - there is NO CPU fallback: every compute entry point fails with
 *     BNF_ERR_NO_DEVICE when no gfx950 device is usable.
 */
#ifndef BNF_H_
#define BNF_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BNF_ABI_VERSION 6

/* limits of the static network description */
#define BNF_MAX_INPUTS   8    /* D  : time + spatial covariates              */
#define BNF_MAX_GROUPS   12   /* feature groups (inputs, fourier_d, seasonal, interactions) */
#define BNF_MAX_LAYERS   8    /* hidden layers                                */
#define BNF_MAX_FREQS    96   /* distinct seasonal frequencies                */
#define BNF_MAX_INTERACT 16

enum {
  BNF_OK = 0,
  BNF_ERR_INVALID = -1,    /* bad argument / unsupported configuration */
  BNF_ERR_NO_DEVICE = -2,  /* no usable HIP device (no CPU fallback exists) */
  BNF_ERR_HIP = -3,        /* a HIP runtime call failed */
  BNF_ERR_STATE = -4       /* call order violated (e.g. train before bind) */
};

enum { BNF_DTYPE_F32 = 0, BNF_DTYPE_BF16 = 1,   /* arithmetic of the dense contractions; accumulation is always f32 */
       /* BASELINE.json configs[4] ("fp8 MFMA dense layers"): the row-panel pipeline with (round 5) FP8 OPERAND STORAGE for
        * the weight-gradient contractions -- the activation copies H_l leave as OCP e4m3, the backward signals dZ_l as OCP
        * e5m2 over a per-member power of two, and dK_l = H_l^T dZ_l runs on the fp8 MFMA -- and (round 6, the folded forms:
        * F + 2 <= padded feature count, i.e. every BASELINE layout) the W x W FORWARD and BACKWARD-DATA contractions on the
        * block-scaled fp8 MFMA (v_mfma_scale_f32_32x32x64_f8f6f4) out of fp8 panels in LDS, weights as e4m3 x 2^5; layer 0
        * and its backward-data stay bf16 (env BNF_FP8_CONTRACT=0 at bnf_create: storage only).  Needs the row-panel pipeline
        * (depth >= 2, padded width 256 / 512 / 1024, <= 128 padded features): bnf_create refuses other shapes. */
       BNF_DTYPE_FP8 = 2,
       /* f32 storage, accumulation and epilogues like BNF_DTYPE_F32, but the contractions run on SPLIT-bf16 MFMAs: every f32
        * operand is split in registers into two bf16 pieces (16 operand bits) and hi*hi + hi*lo + lo*hi are summed by three
        * bf16 MFMAs -- products good to ~5e-6 of the largest output (exact chain: 1e-7), the three reference goldens (< 1e-4)
        * hold, 1.8x the speed of the exact f32 MFMA chain.  compute_dtype 'fp32_split' in the Python layer -- also what its
        * estimators run when no dtype is given (both f32-class engines hold SURVEY 8d's fp32 gates verbatim); an explicit
        * 'fp32' is BNF_DTYPE_F32, the exact v_mfma_f32_32x32x2_f32 arithmetic (ABI 6; ABI 5's Python layer had mapped the
        * NAME 'fp32' here). */
       BNF_DTYPE_F32S = 3 };
enum { BNF_OBS_NORMAL = 0, BNF_OBS_NB = 1, BNF_OBS_ZINB = 2 }; /* models.py:30-33 */
enum { BNF_MODE_MAP = 0, BNF_MODE_VI = 1 };       /* MLE = MAP with prior_weight 0 (spatiotemporal.py:551) */

/* feature-group kinds, order of models.py:242-247 */
enum { BNF_GROUP_INPUT = 0, BNF_GROUP_FOURIER = 1, BNF_GROUP_SEASONAL = 2, BNF_GROUP_INTERACT = 3 };

/* Static description of the network + run.  Mirrors `model_args`
 * (spatiotemporal.py:360-370) plus the arguments of ensemble_map / ensemble_vi
 * (inference.py:510-522, 626-639).  Offsets index the packed per-member
 * parameter vector whose leaf order is the reference's `params_` tuple
 * (models.py:95-103 + sorted flax leaves; bayesnf_amd/spec.py). */
typedef struct bnf_config {
  int32_t abi_version;      /* BNF_ABI_VERSION */
  int32_t device;           /* HIP device ordinal */
  int32_t dtype;            /* BNF_DTYPE_* */
  int32_t obs_model;        /* BNF_OBS_* */
  int32_t mode;             /* BNF_MODE_* */

  /* network (models.py:197-273) */
  int32_t n_inputs;         /* D */
  int32_t width;            /* W, 1..8192 (the kernels run at the next multiple of 64 on zero-padded
                               copies of the width-dependent leaves; parameters, gradients and
                               optimiser state keep the reference's shapes) */
  int32_t depth;            /* hidden layers, 1..BNF_MAX_LAYERS */
  int32_t n_features;       /* F */
  int32_t n_params;         /* P */
  int32_t n_groups;
  int32_t group_kind[BNF_MAX_GROUPS];
  int32_t group_arg[BNF_MAX_GROUPS];        /* input column for FOURIER */
  int32_t group_ncols[BNF_MAX_GROUPS];
  int32_t group_col0[BNF_MAX_GROUPS];
  int32_t group_scale_off[BNF_MAX_GROUPS];  /* feature_inv_sp_scale{i} */
  int32_t fourier_degree[BNF_MAX_INPUTS];
  float   input_scale[BNF_MAX_INPUTS];      /* float32(input_scales) */
  int32_t n_freqs;
  float   freq[BNF_MAX_FREQS];              /* make_seasonal_frequencies, float32 */
  float   harmonic[BNF_MAX_FREQS];
  int32_t n_interact;
  int32_t interact[BNF_MAX_INTERACT][2];
  int32_t off_log_noise_scale, off_shape, off_inflated;   /* params[0..2] */
  int32_t off_bias[BNF_MAX_LAYERS + 1];     /* Dense_l/bias ; [depth] = output layer */
  int32_t off_kernel[BNF_MAX_LAYERS + 1];   /* Dense_l/kernel (in,out) row-major */
  int32_t off_layer_scale[BNF_MAX_LAYERS];  /* inv_sp_layer_scale{l} */
  int32_t off_output_scale;
  int32_t off_lsa;                          /* log_scale_adjustment (D) */
  int32_t off_act_weight;                   /* logit_activation_weight */

  /* run (inference.py:510-522 / 626-639) */
  int64_t n_rows;           /* N training rows held in X / y */
  int64_t batch;            /* B rows per step (== N: full batch, no shuffling) */
  int32_t members;          /* ensemble members on THIS device */
  int64_t member_offset;    /* global id of local member 0: random streams are keyed
                               by the global id, so results do not depend on sharding */
  int32_t vi_samples;       /* S = sample_size_divergence (VI), else 1 */
  int32_t forward_only;     /* 1: handle is used for bnf_forward / quantiles only
                               (no backward buffers are carved, bnf_train refuses) */
  int32_t pipeline;         /* train-step kernels.  0 auto: one kernel per layer, with the last hidden
                               layer + output layer + likelihood + its backward in ONE kernel when
                               the width is 64/128/256 (512: bf16 only).  1: one kernel per layer and
                               every activation materialised (validation; bnf_debug_activation can
                               read all of them).
                               3: row-panel forward + backward kernel (bnf_panel.h: bf16, depth 2,
                               width 256/512, <= 128 features) -- what 0 selects where it applies */
  float   learning_rate;
  float   prior_weight;     /* 1 MAP, 0 MLE (inference.py:561-569) */
  float   kl_weight;        /* VI (inference.py:689-702) */
  uint64_t seed;
} bnf_config;

typedef struct bnf_handle bnf_handle;

/* ---- lifecycle ----------------------------------------------------------- */
int bnf_abi_version(void);
const char* bnf_last_error(void);

/* Validates cfg, selects the device, precomputes launch geometry. */
int bnf_create(const bnf_config* cfg, bnf_handle** out);
void bnf_destroy(bnf_handle* h);

/* Sizes (bytes) of the caller-provided device buffers. */
size_t bnf_workspace_bytes(const bnf_handle* h);  /* activations, gradients, packed weights */
size_t bnf_state_bytes(const bnf_handle* h);      /* optimiser state: MAP 2*E*P f32 (m,v); VI 4*E*P */
size_t bnf_param_bytes(const bnf_handle* h);      /* MAP E*P f32 ; VI 2*E*P (mu then rho) */
/* Device memory the engine has allocated ITSELF so far (everything else is the caller's): today only the work
 * buffers of bnf_row_keys -- 4 x members x n_rows x 4 bytes + (members + 1) x 4 + the radix sort's scratch --
 * allocated at the first epoch that draws its shuffles on the device, all or nothing (a failed allocation
 * returns BNF_ERR_HIP from bnf_train and leaves nothing behind), freed by bnf_destroy.  0 before that. */
size_t bnf_owned_bytes(const bnf_handle* h);

/* Attach device buffers.  X: (N, D) f32 row-major, y: (N,) f32 (replicated
 * closed-over constants of ensemble_map, inference.py:553-554).  Zeroes the
 * workspace and precomputes the seasonal feature table (models.py:62-76; the
 * features of the raw time index are data-constant).  */
int bnf_bind(bnf_handle* h, void* params /*DEVICE*/, void* opt_state /*DEVICE*/,
             void* workspace /*DEVICE*/, const float* X /*DEVICE*/,
             const float* y /*DEVICE*/, void* stream);

/* ---- training -------------------------------------------------------------- */
/* Initial values (inference.py:399-427 MAP/MLE ; :203-231 VI): Dense kernels ~
 * TruncatedNormal(0,1,[-2,2]) from the counter RNG keyed by (seed, global member,
 * index); log_noise_scale = log_noise_init (MAP: log(nanstd(y)/2), VI: 0);
 * everything else 0; VI rho = softplus^-1(0.3).  Resets optimiser state + step. */
int bnf_init_params(bnf_handle* h, float log_noise_init);

/* The reference's OWN initial parameters for the user's seed, drawn on the device from their keys (what fit() uses;
 * bnf_init_params above draws same-law values from the engine's generator).  MAP / MLE (inference.py:399-427) and
 * the VI surrogate means (:203-231) are one JointDistribution sample per member: one key per leaf
 * (bayesnf_amd/jaxseed.py map_leaf_keys / vi_mean_leaf_keys restate the split chain on the host), Dense kernels
 * ~ TruncatedNormal(0, 1, -2, 2) through jax.random.truncated_normal -- threefry2x32 bits, uniform on
 * [erf(-sqrt2), erf(sqrt2)), sqrt2 erfinv, clip -- every other leaf 0, log_noise_scale = log_noise_init;
 * VI: rho = softplus^-1(0.3).  Resets the optimiser state and the step counter like bnf_init_params.
 *   leaf_keys    DEVICE uint32 (members, n_leaves, 2)
 *   leaf_offsets HOST int32 (n_leaves + 1): offsets of the packed leaves, [0] = 0, [n_leaves] = P; n_leaves <= 64 */
int bnf_init_params_keys(bnf_handle* h, const uint32_t* leaf_keys, const int32_t* leaf_offsets, int32_t n_leaves,
                         float log_noise_init);

/* ensemble_map._run / tfp.vi.fit_surrogate_posterior_stateless (inference.py:
 * 577-619 / 727-738): `num_epochs` x (N // B) Adam steps for every local member,
 * enqueued back to back with no host round trip.  losses: DEVICE (members,
 * num_epochs) f32, receives the per-epoch mean of the pre-update step losses
 * (inference.py:614); for VI one "epoch" is one step and the value is already
 * multiplied by kl_weight (inference.py:758).  `epoch0` = index of the first
 * epoch (continuation of an earlier call; keys the shuffles). */
int bnf_train(bnf_handle* h, int64_t epoch0, int64_t num_epochs, float* losses /*DEVICE*/);

/* VI only: draw `n_draws` parameter vectors per member from the fitted
 * surrogate (inference.py:741-745).  out: DEVICE (n_draws, members, P) f32. */
int bnf_vi_posterior_draws(bnf_handle* h, int32_t n_draws, float* out /*DEVICE*/);

/* The reference's OWN minibatch shuffles for MAP / MLE (optional; without it every member shuffles each
 * epoch with the engine's keyed Feistel bijection -- same law, other numbers).  ensemble_map
 * (inference.py:571-575, 593-597, 622) permutes the data set per member and per epoch with
 * jax.random.permutation(permute_seed, N), permute_seed from the member's key chain; bayesnf_amd/jaxseed.py
 * restates that chain on the host.
 *   tables DEVICE int32 (n_epochs, members, (N / batch) * batch): row ids of the epochs
 *          [epoch0, epoch0 + n_epochs) of bnf_train's epoch counter, step s of an epoch reading
 *          columns [s * batch, (s + 1) * batch); values in [0, N).  Caller-owned, must stay alive while
 *          those epochs are enqueued AND executing; epochs outside the range use the engine's shuffle.
 * NULL restores the engine's shuffle.  Full-batch handles ignore it (no shuffle there). */
int bnf_row_tables(bnf_handle* h, const int32_t* tables, int64_t epoch0, int64_t n_epochs);

/* The same shuffles drawn ON THE DEVICE from their keys (what fit() uses: no per-epoch host work, no row-id upload --
 * at 10^7 rows a host-side table is 40 MB per member and epoch).  jax.random.permutation(permute_seed, N) is
 * `rounds` = ceil(3 ln N / ln(2^32 - 1)) times { permute_seed, sub = split(permute_seed); stable sort of the current
 * order by random_bits(sub, (N,)) } (jax/_src/random.py _shuffle); the caller supplies the sub keys
 * (bayesnf_amd/jaxseed.py map_shuffle_subkeys), the engine draws the bits (threefry2x32) and sorts (radix, stable)
 * when an epoch starts, on the handle's stream.
 *   keys DEVICE uint32 (n_epochs, members, rounds, 2) for the epochs [epoch0, epoch0 + n_epochs); caller-owned,
 *        alive while those epochs are enqueued and executing.  BNF_ERR_INVALID if `rounds` is not jax's count for N.
 * Work buffers (4 x members x N x 4 bytes + sort scratch) are allocated by the engine at the first such epoch
 * (the only allocation the engine makes itself: bnf_owned_bytes reports it) and freed by bnf_destroy.
 * BNF_ERR_INVALID when members x N exceeds 2^31 - 1 (32-bit sort offsets): use bnf_row_tables or the engine's
 * index-free shuffle for such fits.  A table from bnf_row_tables covering the same epoch wins.  NULL switches it off.
 * VI handles (ABI 6): ensemble_vi draws ONE batch per optimisation step, shared by every member --
 * `jax.random.permutation(seed, arange(N))[:batch_size]` with the seed tfp hands `target_log_prob_fn` at that step
 * (inference.py:704-709) -- so `keys` is uint32 (n_steps, 1, rounds, 2) for the steps [epoch0, epoch0 + n_steps)
 * (bayesnf_amd/jaxseed.py vi_batch_subkeys), the permutation is drawn when the step is enqueued and its first `batch`
 * entries are the rows of every member; work buffers 4 x N x 4 bytes + sort scratch. */
int bnf_row_keys(bnf_handle* h, const uint32_t* keys, int64_t epoch0, int64_t n_epochs, int32_t rounds);

/* The reference's OWN random stream for the VI noise (optional; without it the noise comes from the
 * engine's counter-based generator -- same law, other numbers).  tfp.vi.fit_surrogate_posterior_stateless
 * (inference.py:727-738) draws, at every step, `vi_samples` joint samples of the surrogate, each leaf
 * with jax.random.normal(key, (members, *leaf shape)); ensemble_vi's posterior draws (:741-753) likewise.
 * The keys are pure functions of the user's seed (threefry split / fold_in chains: bayesnf_amd/jaxseed.py
 * computes them on the host once per fit); the normals themselves are generated on the device.
 *   step_keys DEVICE uint32 (n_steps, vi_samples, n_leaves, 2): row i serves the i-th bnf_train step
 *             counted from this call; training beyond the table fails with BNF_ERR_STATE
 *   draw_keys DEVICE uint32 (n_draws, n_leaves, 2) for bnf_vi_posterior_draws
 *   leaf_offsets HOST int32 (n_leaves + 1): offsets of the parameter leaves, in the reference's order
 * Both tables are caller-owned and must stay alive; NULL, NULL restores the engine's generator.
 * Install them AFTER bnf_init_params / bnf_bind: both reset the step counter and drop installed tables. */
int bnf_vi_noise_keys(bnf_handle* h, const uint32_t* step_keys, int64_t n_steps, const uint32_t* draw_keys,
                      int64_t n_draws, const int32_t* leaf_offsets, int32_t n_leaves);

/* ---- prediction ------------------------------------------------------------ */
/* forecast_inner over all members (inference.py:103-126,129-200): theta is
 * DEVICE (n_members, P) f32 (any count; processed in chunks), Xnew DEVICE
 * (n_rows, D) f32.  loc: DEVICE (n_members, n_rows) f32 = network output;
 * aux: DEVICE (n_members, 3) f32 = {noise scale 0.01+exp(lns), softplus(shape),
 * sigmoid(inflated_loc_probs)}.  Does not touch the training state. */
int bnf_forward(bnf_handle* h, const float* theta, int64_t n_members,
                const float* Xnew, int64_t n_rows, float* loc, float* aux);

/* Quantiles of the equal-weight mixture of Normals over members, per row
 * (inference.py:42-100).  means DEVICE (n_members, n_rows), scales DEVICE
 * (n_members,), q HOST (n_q,), out DEVICE (n_q, n_rows).  approximate=0:
 * Chandrupatla root of mean_e Phi((x-mu_e)/sigma_e) - q on
 * [min mu - 5 max sigma, max mu + 5 max sigma], value tolerance 1e-5, <= 60
 * iterations.  Where the f32 grid around the root is coarser than that tolerance
 * allows (mu = 1e5 with sigma = 0.01: adjacent floats are 0.78 sigma apart) the
 * iterations run out on a bracket of two adjacent floats and the result is the
 * one of them with the smaller residual: the root lies within one f32 step of it.
 * approximate=1: moment-matched Normal, mean + sqrt(var) Phi^-1(q) with
 * mean = mean_e mu_e first and then var = mean_e (sigma_e^2 + (mu_e - mean)^2),
 * centred, both f64 with the members in order, the result rounded to f32 (the
 * one-pass form mean(sigma^2 + mu^2) - mean^2 cancels at the data's own scale). */
int bnf_normal_mixture_quantiles(bnf_handle* h, const float* means, const float* scales,
                                 int64_t n_members, int64_t n_rows, const float* q,
                                 int32_t n_q, int32_t approximate, float* out);

/* Count observation models (handle created with BNF_OBS_NB / BNF_OBS_ZINB):
 * per-member forecast means and quantiles of the equal-weight mixture over members
 * (inference.py:271-333 and :497-502; TFP NegativeBinomial / ZeroInflatedNegativeBinomial
 * mean, stddev, cdf).  loc DEVICE (n_members, n_rows) and aux DEVICE (n_members, 3) as
 * written by bnf_forward; means DEVICE (n_members, n_rows) out; q HOST (n_q,) in (0,1);
 * out DEVICE (n_q, n_rows) = ceil of the Chandrupatla root of mean_e cdf_e(x) - q on
 * [0, max mean + 1.1 rsqrt(1-q) max stddev] (value tolerance 1e-5, <= 60 iterations),
 * 0 where mean_e pmf_e(0) > q.  n_q = 0: means only. */
int bnf_count_mixture_quantiles(bnf_handle* h, const float* loc, const float* aux,
                                int64_t n_members, int64_t n_rows, const float* q,
                                int32_t n_q, float* means, float* out);

/* Posterior-predictive SAMPLE PATHS of the equal-weight mixture over members: what the reference draws with
 * `.sample()` on the TFP distribution its `likelihood_model()` returns (spatiotemporal.py:433-468; models.py:160-191
 * tfd.Normal / NegativeBinomial / ZeroInflatedNegativeBinomial), here as JOINT draws: sample path s picks ONE member
 * c_s = floor(u n_members) for all rows, then draws every row independently from that member's distribution
 * (observation model of the handle; NORMAL N(loc, aux[0]); NB total_count = 1 / aux[1], logits = -log aux[1] -
 * log softplus(loc), drawn as Poisson(Gamma(total_count, scale e^logits)); ZINB: 0 with probability aux[2]).
 *   loc DEVICE (n_members, n_rows) and aux DEVICE (n_members, 3) as written by bnf_forward
 *   out DEVICE (n_samples, n_rows) f32 (counts above 2^24 rounded to the nearest float)
 *   NaN: a NaN parameter of the drawn member gives a NaN draw; a rate beyond the f32 range gives +inf.  The parameters
 *     are loc[c_s, r] (that row only) and the aux entries the model reads (NORMAL aux[0]; NB aux[1]; ZINB aux[1], aux[2]:
 *     every row of the path); the zero inflation does not replace a NaN, and keeps its 0 beside +inf.
 *   row0, sample0: global index of loc's first column / of out's first row.  The value at (sample s, row r) is a pure
 *     function of (seed, sample0 + s, row0 + r, loc[c_s, r], aux[c_s]): a caller may cut rows and samples into chunks of
 *     any size and gets the bits of the one big call.  row0 + n_rows <= 2^56, sample0 + n_samples <= 2^32.
 * Counter layout (Philox4x32-10, key = seed; stream ids of their own beside the training streams, bnf_device.h):
 *   member of path s:  (s, 0, 0, STREAM_PRED_COMPONENT), word 0
 *   draw at (s, r):    (r bits 0..31, s, slot << 16 | trial, STREAM_PRED_DRAW | r bits 32..55 << 8); slot 0 the Normal
 *     draw and the zero-inflation uniform, slot 1 the Gamma proposals (Marsaglia-Tsang), slot 2 the Poisson uniforms
 *     (inversion below rate 10, PTRS above); every rejection loop stops after 64 proposals (bnf_sampling.h).
 * Runs on the handle's stream, does not touch the training state. */
int bnf_predictive_samples(bnf_handle* h, const float* loc, const float* aux, int64_t n_members, int64_t n_rows,
                           int64_t n_samples, uint64_t seed, int64_t row0, int64_t sample0, float* out);

/* Totals of the same sample paths over groups of rows, without materialising the draws: out[s][g] = the f64 sum over
 * the rows of group g of the f32 values bnf_predictive_samples writes for (seed, sample0 + s, row0 + r).  The reference
 * has no counterpart (it would sum `.sample()` on the host).  Deterministic: no floating-point atomics, the order of
 * every sum depends only on the grouping -- two calls give the same bits, counts are exact below 2^53.
 *   seg_offsets DEVICE int32 (n_groups + 1), seg_rows DEVICE int32 (n_rows): the rows sorted by group as CSR; group g
 *     owns seg_rows[seg_offsets[g] .. seg_offsets[g + 1]), [0] = 0, [n_groups] = n_rows, every row once (empty groups
 *     allowed: total 0).  Entries of seg_rows outside [0, n_rows) add nothing.
 *   work DEVICE, work_bytes: per-tile partial sums, 16 bytes x ceil(n_rows / BNF_GROUP_TILE) per sample path; the
 *     samples are processed in as many passes as the buffer asks for (BNF_ERR_INVALID below one path's worth)
 *   out DEVICE (n_samples, n_groups) f64 */
#define BNF_GROUP_TILE 1024
int bnf_predictive_group_sums(bnf_handle* h, const float* loc, const float* aux, int64_t n_members, int64_t n_rows,
                              const int32_t* seg_offsets, const int32_t* seg_rows, int64_t n_groups, int64_t n_samples,
                              uint64_t seed, int64_t row0, int64_t sample0, void* work, size_t work_bytes, double* out);

/* The same sample paths and group totals with WEIGHTS on the members (the weights bnf_stacking_weights finds): the
 * arguments of bnf_predictive_samples / bnf_predictive_group_sums plus
 *   cum_weights DEVICE (n_members,) f64: the running sum of the member weights, nondecreasing, last entry 1.
 * Path s takes the same Philox word as the equal-weight call, u = word / 2^32, and the member c_s = #{m : cum[m] <= u},
 * clamped to n_members - 1 (found by bisection: a cum out of order can only pick another member, never an index outside
 * loc); every draw at (s, r) then uses the counters of the equal-weight call, so weights that sit on one member give the
 * bits of that member alone.  u moves in steps of 2^-32: a member whose weight is below 2^-32 is never drawn.
 * cum_weights == NULL gives the bits of the unweighted call.  Run on the handle's stream, do not touch the training
 * state, work on forward-only handles. */
int bnf_predictive_samples_weighted(bnf_handle* h, const float* loc, const float* aux, int64_t n_members, int64_t n_rows,
                                    int64_t n_samples, uint64_t seed, int64_t row0, int64_t sample0,
                                    const double* cum_weights, float* out);
int bnf_predictive_group_sums_weighted(bnf_handle* h, const float* loc, const float* aux, int64_t n_members, int64_t n_rows,
                                       const int32_t* seg_offsets, const int32_t* seg_rows, int64_t n_groups,
                                       int64_t n_samples, uint64_t seed, int64_t row0, int64_t sample0,
                                       const double* cum_weights, void* work, size_t work_bytes, double* out);

/* LINEAR COMBINATIONS of the rows of the same sample paths, without materialising the draws: weighted means, contrasts
 * (this week minus last week) and overlapping groups (a row in its county, its state and the nation) in the same paths.
 * The reference has no counterpart (it would multiply `.sample()` by a matrix on the host).  loc, aux, row0, sample0 and
 * cum_weights (NULL = equal weights) as for bnf_predictive_group_sums_weighted.
 *   form_offsets DEVICE int32 (n_forms + 1), form_rows DEVICE int32 (nnz), form_coef DEVICE f64 (nnz): a CSR over
 *     POSITIONS; form k owns the positions form_offsets[k] .. form_offsets[k + 1] - 1.  [0] = 0, nondecreasing,
 *     nnz = form_offsets[n_forms], 0 <= nnz < 2^31.  The call reads nnz back from the device (4 bytes), after the checks
 *     below.
 *   out DEVICE (n_samples, n_forms) f64
 * COEFFICIENT: out[s][k] = the f64 sum over the positions p of form k of form_coef[p] * (double)x, x the f32 that
 *   bnf_predictive_samples writes for (seed, sample0 + s, row0 + form_rows[p]), bit for bit.  Each product is one f64
 *   multiply, rounded once and never contracted into the addition that follows.
 * OVERLAP: a row may stand at any number of positions, of the same form or of different ones; every occurrence adds, and
 *   the draw is the same at each (a row at m positions is drawn m times).  A row at no position is never drawn.  A
 *   position whose row lies outside [0, n_rows) adds nothing, whatever its coefficient.
 * EMPTY: a form without positions is 0.0.
 * NaN: a NaN coefficient or a NaN draw makes the value of its own form NaN, and of no other form.
 * DETERMINISM: no floating-point atomics.  The position axis is cut into tiles of BNF_GROUP_TILE and the order of every
 *   sum depends only on form_offsets: two calls give the same bits, and neither sample0 chunking nor the number of passes
 *   that work_bytes forces changes them.  row0 is the global index of loc's first column; the ROW axis cannot be cut
 *   into chunks here, because a form may span all rows: loc holds every row a form names.  When the forms are a
 *   partition of the rows (nnz = n_rows, every row once) and every coefficient is 1.0, out has the bits of
 *   bnf_predictive_group_sums (with cum_weights: of bnf_predictive_group_sums_weighted) for that grouping.
 *   work DEVICE, work_bytes: per-tile partial sums, 16 bytes x ceil(nnz / BNF_GROUP_TILE) per sample path; the samples
 *     are processed in as many passes as the buffer asks for
 * BNF_ERR_INVALID, with nothing launched: n_members, n_rows, n_forms or n_samples < 1, a NULL loc, aux, form_offsets,
 *   form_rows, form_coef, work or out, row0 / sample0 out of range, a negative position count, and a work buffer below one
 *   path's worth.  An unbound handle is BNF_ERR_STATE, as for bnf_predictive_group_sums.
 * Runs on the handle's stream, does not touch the training state, works on forward-only handles. */
int bnf_predictive_combinations(bnf_handle* h, const float* loc, const float* aux, int64_t n_members, int64_t n_rows,
                                const int32_t* form_offsets, const int32_t* form_rows, const double* form_coef,
                                int64_t n_forms, int64_t n_samples, uint64_t seed, int64_t row0, int64_t sample0,
                                const double* cum_weights /* may be NULL */, void* work, size_t work_bytes, double* out);

/* PEAKS and threshold EXCEEDANCES of the same sample paths over groups of rows, without materialising the draws (the
 * reference has no counterpart: it would reduce `.sample()` on the host).  The value at (path s, row r) is the f32 that
 * bnf_predictive_samples writes for (seed, sample0 + s, row0 + r), bit for bit; loc, aux, seg_offsets, seg_rows, row0,
 * sample0 as for bnf_predictive_group_sums.  Per (path s, group g):
 *   out_max DEVICE (n_samples, n_groups) f64: the largest draw over the group's rows (the f32 draw widened: the matrix
 *     is one bnf_sample_summaries takes)
 *   out_argmax DEVICE (n_samples, n_groups) int32 or NULL: the TABLE ROW (an entry of seg_rows) at which that maximum is
 *     first reached.  Tie rule: among equal draws the lowest position of seg_rows wins -- the lowest table row of the
 *     group when the rows ascend inside a group
 *   out_count DEVICE (n_samples, n_groups) f64, NULL iff threshold is NULL: the number of rows of the group whose draw is
 *     strictly greater than threshold[row] (an exact integer)
 *   threshold DEVICE (n_rows,) f32 or NULL: one limit per table row, in the units of the draws
 *   cum_weights DEVICE (n_members,) f64 or NULL: as for bnf_predictive_samples_weighted; NULL takes the integer
 *     floor(u n_members) component of the equal-weight calls
 * NaN rule: a NaN draw enters the maximum as -inf (at its own position) and never exceeds a threshold, so "b beats a iff
 * b.v > a.v, or b.v == a.v and b.pos < a.pos" is a total order and the result does not depend on tile edges, the launch
 * geometry or the number of passes.  Entries of seg_rows outside [0, n_rows) take no part.  Empty-group values: a group
 * without a row that takes part reports max = NaN, argmax = -1, count = 0.
 * Two optional per-row counters, DEVICE (n_rows,) uint32, ZEROED BY THE CALLER and added to with integer atomics only:
 *   peak_count[r] += the number of paths in which row r is its group's argmax
 *   exceed_count[r] += the number of paths whose draw at r is > threshold[r] (needs threshold)
 *   work DEVICE, work_bytes: per-tile pieces, BNF_EXTREMES_WORK_PER_TILE bytes x ceil(n_rows / BNF_GROUP_TILE) per sample
 *     path; the samples are processed in as many passes as the buffer asks for (BNF_ERR_INVALID below one path's worth)
 * Deterministic: no floating-point atomics -- two calls give the same bits.  Runs on the handle's stream, does not touch
 * the training state, works on forward-only handles. */
#define BNF_EXTREMES_WORK_PER_TILE 32
int bnf_predictive_group_extremes(bnf_handle* h, const float* loc, const float* aux, int64_t n_members, int64_t n_rows,
                                  const int32_t* seg_offsets, const int32_t* seg_rows, int64_t n_groups, int64_t n_samples,
                                  uint64_t seed, int64_t row0, int64_t sample0, const double* cum_weights,
                                  const float* threshold, void* work, size_t work_bytes, double* out_max,
                                  int32_t* out_argmax, double* out_count, uint32_t* peak_count, uint32_t* exceed_count);

/* SPELLS above a threshold in the same sample paths, per group of rows, without materialising the draws (the reference
 * has no counterpart: it would loop over `.sample()` on the host).  The value at (path s, row r) is the f32 that
 * bnf_predictive_samples writes for (seed, sample0 + s, row0 + r), bit for bit; loc, aux, seg_offsets, seg_rows, row0,
 * sample0 and cum_weights (NULL = equal weights) as for bnf_predictive_group_extremes.  TIME is the order of the
 * positions of seg_rows inside a group (sort the rows of a group by time: inference.csr_ordered).
 *   threshold DEVICE (n_rows,) f32, required: a position EXCEEDS when its draw is strictly greater than threshold[row].
 *     A NaN draw does not exceed but takes part: it breaks a spell and counts as a step.  An entry of seg_rows outside
 *     [0, n_rows) takes no part: it neither breaks a spell nor counts as a step.
 * Per (path s, group g), each skipped when its pointer is NULL except out_longest:
 *   out_longest DEVICE (n_samples, n_groups) f64: length of the longest run of consecutive exceeding positions, 0 if none
 *   out_longest_row DEVICE (n_samples, n_groups) int32: the TABLE ROW (an entry of seg_rows) at which that run starts;
 *     among equally long runs the earliest wins; -1 if none
 *   out_spells DEVICE (n_samples, n_groups) f64: the number of maximal runs
 *   out_onset_step DEVICE (n_samples, n_groups) f64: the number of participating positions before the first exceeding
 *     one; when the path never exceeds, the number of participating positions of the group (censored at the horizon,
 *     never NaN: bnf_sample_summaries takes the matrix)
 *   out_first_row, out_last_row DEVICE (n_samples, n_groups) int32: table row of the first / last exceeding position, -1
 *     if none
 *   onset_count DEVICE (n_rows,) uint32 or NULL, ZEROED BY THE CALLER, added to with integer atomics only:
 *     onset_count[r] += the number of paths in which r is its group's first exceeding row
 * A group without a participating position reports 0 / -1 / 0 / 0 / -1 / -1.
 * The reduction joins pieces (len, lead, pre, suf, suf_pos, best, best_pos, runs, first, last) in position order with an
 * associative, all-integer operator (bnf_episodes.h): the result does not depend on tile edges, the launch geometry or
 * the number of passes, and two calls give the same bits.  No floating-point atomics.
 *   work DEVICE, work_bytes: per-tile pieces, BNF_EPISODES_WORK_PER_TILE bytes x ceil(n_rows / BNF_GROUP_TILE) per sample
 *     path; the samples are processed in as many passes as the buffer asks for (BNF_ERR_INVALID below one path's worth)
 * BNF_ERR_INVALID also for a NULL threshold or out_longest and for n_members, n_rows, n_groups or n_samples < 1.
 * Runs on the handle's stream, does not touch the training state, works on forward-only handles. */
#define BNF_EPISODES_WORK_PER_TILE 80
int bnf_predictive_group_episodes(bnf_handle* h, const float* loc, const float* aux, int64_t n_members, int64_t n_rows,
                                  const int32_t* seg_offsets, const int32_t* seg_rows, int64_t n_groups, int64_t n_samples,
                                  uint64_t seed, int64_t row0, int64_t sample0, const double* cum_weights,
                                  const float* threshold, void* work, size_t work_bytes, double* out_longest,
                                  int32_t* out_longest_row, double* out_spells, double* out_onset_step,
                                  int32_t* out_first_row, int32_t* out_last_row, uint32_t* onset_count);

/* RUNNING TOTALS of the same sample paths, per group of rows, and when they pass a level, without materialising the
 * draws (the reference has no counterpart: it would loop over `.sample()` and cumsum on the host).  loc, aux,
 * seg_offsets, seg_rows, row0, sample0 and cum_weights (NULL = equal weights) as for bnf_predictive_group_episodes.
 * TIME is the order of the positions of seg_rows inside a group (inference.csr_ordered).  Per path s, group g and
 * position p of g:
 *   run[s][p] = the f64 sum of the draws at the participating positions of g up to and including p.  A draw is the f32
 *     that bnf_predictive_samples writes for (seed, sample0 + s, row0 + row), bit for bit, widened to f64.
 *   An entry of seg_rows outside [0, n_rows) takes no part: its run is the value carried so far (0 at a group's start)
 *     and it is not a step.  A NaN draw takes part: it makes every later run of its group NaN, as a cumulative sum does,
 *     and it counts as a step.
 *   out_total DEVICE (n_samples, n_groups) f64, required: run at the group's last position; 0 for a group without a
 *     participating position
 *   out_running DEVICE (n_samples, n_rows) f64 or NULL: run, column = POSITION of seg_rows (not table row)
 *   level DEVICE (n_groups,) f64 or NULL: one level per group.  The CROSSING POSITION of (s, g) is the first participating
 *     position with run > level[g]; the comparison is strict, in f64, and false for NaN.  With a level, each skipped
 *     when its pointer is NULL:
 *   out_cross_step DEVICE (n_samples, n_groups) f64: the number of participating positions before the crossing position;
 *     when the path never crosses, the number of participating positions of the group (censored at the horizon, never
 *     NaN: bnf_sample_summaries takes the matrix)
 *   out_cross_row DEVICE (n_samples, n_groups) int32: the TABLE ROW of the crossing position, -1 when the path never
 *     crosses
 *   cross_count, above_count DEVICE (n_rows,) uint32, ZEROED BY THE CALLER, added to with integer atomics only:
 *     cross_count[r] += the number of paths in which r is its group's crossing row
 *     above_count[r] += the number of paths with run > level at r's position
 *     (the running total of a NORMAL handle can come back under the level: above_count is not the running sum of
 *     cross_count)
 * A group without a participating position reports total 0, cross_step 0, cross_row -1.
 * One kernel over tiles of BNF_GROUP_TILE positions, no work buffer: a group that leaves its tile through the far edge
 * is finished by the block of the tile it starts in, which walks on over the following tiles; no workgroup waits for
 * another (bnf_cumulative.h).  A long group is therefore parallel over the samples only.
 * DETERMINISM: no floating-point atomics; two calls give the same bits.  The bits of every output depend only on the
 * seed, sample0 + s, row0, loc, aux, cum_weights, level and the CSR arrays: not on n_samples, on how the samples are cut
 * into calls, on the launch geometry or on which output pointers are NULL.  They may depend on where a group lies on the
 * position axis: the order of the f64 additions follows the tiling, as for bnf_predictive_group_sums.  For NB and ZINB
 * every sum is an exact integer below 2^53, so the order plays no part.
 * BNF_ERR_INVALID also for a NULL out_total, for any of out_cross_step, out_cross_row, cross_count, above_count non-NULL
 * while level is NULL, and for n_members, n_rows, n_groups or n_samples < 1; nothing is written then.
 * Runs on the handle's stream, does not touch the training state, works on forward-only handles. */
int bnf_predictive_group_cumulative(bnf_handle* h, const float* loc, const float* aux, int64_t n_members, int64_t n_rows,
                                    const int32_t* seg_offsets, const int32_t* seg_rows, int64_t n_groups,
                                    int64_t n_samples, uint64_t seed, int64_t row0, int64_t sample0,
                                    const double* cum_weights, const double* level, double* out_total,
                                    double* out_running, double* out_cross_step, int32_t* out_cross_row,
                                    uint32_t* cross_count, uint32_t* above_count);

/* MOVING-WINDOW TOTALS of the same sample paths, per group of rows: the total over the last w positions at every
 * position, its peak over the group and how often it lies above a limit, without materialising the draws (the reference
 * has no counterpart).  loc, aux, seg_offsets, seg_rows, row0, sample0 and cum_weights (NULL = equal weights) as for
 * bnf_predictive_group_cumulative.  TIME is the order of the positions of seg_rows inside a group
 * (inference.csr_ordered).  window is an int32 w >= 1, one per call.  Group g has the positions o0 .. o1 - 1, and p is
 * one of them:
 *   DRAW.  x[s][p] is the f32 that bnf_predictive_samples writes for (seed, sample0 + s, row0 + row), bit for bit,
 *     widened to f64.
 *   ENTRIES THAT TAKE NO PART.  An entry of seg_rows outside [0, n_rows) takes no part.  It occupies a slot of the
 *     window, because windows are counted in positions.  It adds nothing, is never NaN and is never a candidate.
 *   WINDOW SUM.  win[s][p] is the f64 sum of the draws at the participating positions in max(o0, p - w + 1) .. p.  The
 *     window is clipped at the group's start.
 *   NaN DRAWS.  A NaN draw makes exactly the windows that contain it NaN.  The window ending w positions later is finite
 *     again.  This is deliberately not the behaviour of a naive sliding sum, which stays NaN for ever.
 *   CANDIDATE.  Position p is a candidate if it takes part and p - o0 + 1 >= min(w, o1 - o0).  These are the full-length
 *     windows.  For a group shorter than w, the candidate is the one window that is the whole group, which ends at its
 *     last position.  With w >= the group's size, the only candidate window is therefore the group total.
 *   PEAK.  peak[s][g] is the largest non-NaN win over the candidates of g; peak_row is the TABLE ROW of the earliest
 *     position at which it is reached.  With no candidate, or none that is not NaN, the results are NaN and -1.  The
 *     total order is that of bnf_predictive_group_extremes: value descending, position ascending, NaN entering as -inf.
 *   THRESHOLD.  threshold DEVICE (n_groups,) f64 or NULL, one limit per group, like `level`.  The test is
 *     win > threshold[g]: strict, in f64, false for NaN.  With a threshold:
 *       count[s][g] is the number of candidates above it, as an f64;
 *       exceed_count[r] += the paths whose candidate window ending at r's position is above it.
 * Outputs, each skipped when its pointer is NULL except out_peak:
 *   out_peak DEVICE (n_samples, n_groups) f64, required
 *   out_peak_row DEVICE (n_samples, n_groups) int32
 *   out_window DEVICE (n_samples, n_rows) f64: win, column = POSITION of seg_rows (not table row); written at every
 *     position, candidate or not (the clipped sum)
 *   out_count DEVICE (n_samples, n_groups) f64, needs threshold
 *   peak_count DEVICE (n_rows,) uint32, ZEROED BY THE CALLER: += the paths whose peak window ends at r
 *   exceed_count DEVICE (n_rows,) uint32, ZEROED BY THE CALLER, needs threshold
 * A group without a candidate reports peak NaN, peak_row -1, count 0.
 * One kernel over tiles of BNF_GROUP_TILE positions, no work buffer: what is summed from a group's start is
 * x[p] - x[p - w]; the draw that leaves comes from the draws of the block's current and previous tile kept in LDS, or,
 * further back, is drawn again: a position costs one draw for w <= BNF_GROUP_TILE and at most two beyond
 * (bnf_windows.h).  A group that leaves its tile through the far edge is finished by the block of the tile it starts in;
 * no workgroup waits for another.  A long group is therefore parallel over the samples only.  Draws are taken to be
 * finite or NaN.
 * DETERMINISM: no floating-point atomics; two calls give the same bits.  The bits of every output depend only on the
 * seed, sample0 + s, row0, loc, aux, cum_weights, window, threshold and the CSR arrays: not on n_samples, on how the
 * samples are cut into calls, on the launch geometry or on which output pointers are NULL.  They may depend on where a
 * group lies on the position axis: the order of the f64 additions follows the tiling.  For NB and ZINB everything is an
 * exact integer below 2^53, so the order plays no part.
 * BNF_ERR_INVALID, with nothing written, for a NULL out_peak, for window < 1, for out_count or exceed_count non-NULL
 * while threshold is NULL, and for n_members, n_rows, n_groups or n_samples < 1.
 * Runs on the handle's stream, does not touch the training state, works on forward-only handles. */
int bnf_predictive_group_windows(bnf_handle* h, const float* loc, const float* aux, int64_t n_members, int64_t n_rows,
                                 const int32_t* seg_offsets, const int32_t* seg_rows, int64_t n_groups, int64_t n_samples,
                                 uint64_t seed, int64_t row0, int64_t sample0, const double* cum_weights, int32_t window,
                                 const double* threshold, double* out_peak, int32_t* out_peak_row, double* out_window,
                                 double* out_count, uint32_t* peak_count, uint32_t* exceed_count);

/* SCORES of held-out observations y against the ensemble: what a user of the reference computes on the host from
 * `likelihood_model()` (`.log_prob`, `.cdf`; spatiotemporal.py:433-468) plus the scores of the equal-weight mixture over
 * members.  loc, aux as for bnf_predictive_samples, with the same per-member laws (observation model of the handle);
 * y DEVICE (n_rows,) f32.  Four outputs, each skipped when its pointer is NULL:
 *   member_ll DEVICE (n_members,) f64: sum over the rows with a finite y of log p_m(y_r) -- the per-member `log_prob`,
 *     evaluated in the forms of the training loss (bnf_scoring.h), so that held-out and training likelihood agree
 *   lpd DEVICE (n_rows,) f32: log((1 / M) sum_m p_m(y_r)), formed in log space: finite where every p_m underflows
 *   pit DEVICE (2, n_rows) f32: [0] = F(y_r), [1] = F(y_r-) of the mixture (NORMAL: equal; counts: F at the integer
 *     below y_r, 0 at y_r = 0): a randomised PIT is uniform on [pit[1], pit[0]]
 *   crps DEVICE (n_rows,) f32: NORMAL handles only (BNF_ERR_INVALID if non-NULL on a count handle), the closed form for
 *     a Normal mixture, (1 / M) sum_i A(y - mu_i, s_i) - (1 / (2 M^2)) sum_ij A(mu_i - mu_j, sqrt(s_i^2 + s_j^2)),
 *     A(m, s) = m (2 Phi(m / s) - 1) + 2 s phi(m / s)
 * A row whose y is NaN or infinite gives NaN in every per-row output and adds nothing to member_ll.
 * Every term is f32, every sum over members, pairs of members and rows f64 in an order the shapes fix: no floating-point
 * atomics, two calls give the same bits.
 *   work DEVICE, work_bytes: partial sums, needed for member_ll and crps only (may be NULL otherwise):
 *       8 * n_members * ceil(n_rows / BNF_SCORE_ROW_TILE)                                             if member_ll
 *     + 8 * n_rows * min(ceil(ceil(n_members / BNF_SCORE_MEMBER_CHUNK) / 2), BNF_SCORE_MAX_SLOTS)     if crps
 *     bytes; BNF_ERR_INVALID below that, and for n_members < 1 or n_rows < 1.
 * Runs on the handle's stream, does not touch the training state, works on forward-only handles. */
#define BNF_SCORE_ROW_TILE 1024
#define BNF_SCORE_MEMBER_CHUNK 8
#define BNF_SCORE_MAX_SLOTS 64
int bnf_predictive_scores(bnf_handle* h, const float* loc, const float* aux, int64_t n_members, int64_t n_rows,
                          const float* y, void* work, size_t work_bytes,
                          double* member_ll, float* lpd, float* pit, float* crps);

/* The RANKED PROBABILITY SCORE of held-out counts y against the ensemble (handle created with BNF_OBS_NB / BNF_OBS_ZINB;
 * BNF_ERR_INVALID on a NORMAL handle, whose CRPS bnf_predictive_scores has): the CRPS of a count forecast,
 *   rps_r = sum_{k >= 0} (F_r(k) - 1{k >= y_r})^2,  F_r(k) = (1 / M) sum_m F_{m,r}(k)
 * with the per-member laws of bnf_predictive_samples.  loc, aux, y as for bnf_predictive_scores; rps DEVICE (n_rows,) f32.
 * The sum is taken term by term on a per-row window [a_r, b_r) and in closed form outside it, where every member's lower
 * (below a_r) or upper (from b_r) tail is under 1e-9 (bnf_rps.h: how the window is found, the truncation bound).
 * A row whose window is longer than BNF_RPS_MAX_TERMS gives NaN -- the work per row is bounded; a mean of 1e6 at
 * total_count 0.05 would need 3e8 terms, and a strided or quadrature form for such rows is out of scope.  A row whose y is
 * NaN, infinite, negative or not an integer gives NaN.  n_members <= BNF_RPS_MAX_MEMBERS (the members' running pmf and cdf
 * live in LDS); BNF_ERR_INVALID above that, and for n_members < 1 or n_rows < 1.
 * Everything after the f32 softplus is f64; every sum is in an order the shapes fix: no floating-point atomics, two calls
 * give the same bits.  Runs on the handle's stream, does not touch the training state, works on forward-only handles. */
#define BNF_RPS_MAX_TERMS (1 << 20)
#define BNF_RPS_MAX_MEMBERS 2048
int bnf_count_rps(bnf_handle* h, const float* loc, const float* aux, int64_t n_members, int64_t n_rows,
                  const float* y, float* rps);

/* The MARGINAL FORECAST OF THE WEIGHTED MIXTURE sum_m w_m p_m: the four calls above with member weights (the weights
 * bnf_stacking_weights finds), each with the arguments of its sibling plus
 *   weights DEVICE (n_members,) f64, w_m >= 0, sum_m w_m = 1 -- the layout bnf_stacking_weights writes, so learned weights
 *     pass through without a host trip.  NULL is BNF_ERR_INVALID: the unweighted call has its own name.
 * bnf_normal_mixture_quantiles_weighted: approximate=0 the Chandrupatla root of sum_m w_m Phi((x - mu_m) / sigma_m) - q
 *   (bracket, tolerances and iteration cap of the unweighted call); approximate=1 the moment-matched Normal with
 *   mean = sum w mu, then var = sum w (sigma^2 + (mu - mean)^2), centred and f64 as in the unweighted call.
 * bnf_count_mixture_quantiles_weighted: ceil of the root of sum_m w_m cdf_m(x) - q, 0 where sum_m w_m pmf_m(0) > q; the
 *   per-member `means` are unchanged.
 * bnf_predictive_scores_weighted: lpd = log sum_m w_m p_m(y_r) (log space, running max), pit = the weighted mixture CDF at
 *   y_r and just below it, crps (NORMAL only) = sum_i w_i A(y - mu_i, s_i) - [sum_{j<i} w_i w_j A(mu_i - mu_j,
 *   sqrt(s_i^2 + s_j^2)) + sum_i w_i^2 s_i / sqrt(pi)].  No member_ll: it is per member, weights do not touch it.  work:
 *   the crps part of bnf_predictive_scores' formula only.
 * bnf_count_rps_weighted: F_r = sum_m w_m F_{m,r}, P0 = sum_m w_m pi_m; window, eps, cap and BNF_RPS_MAX_MEMBERS as for
 *   bnf_count_rps (a weighted mean of tails that are each below eps is below eps: bnf_rps.h).
 * Every sum over members is f64 -- w_m times the f32 term converted to double -- in an order the shapes fix, no
 * floating-point atomics: two calls give the same bits.  The weights are NOT validated (the library cannot read them
 * without a sync): weights off the simplex give meaningless numbers, never an access outside loc / aux / weights.  A
 * member of weight exactly 0 adds nothing to any sum but still widens the quantile bracket and the RPS window (it can cap
 * a row), and a NaN in its parameters still propagates: drop such members before the call (the Python wrappers do).
 * Run on the handle's stream, do not touch the training state, work on forward-only handles. */
int bnf_normal_mixture_quantiles_weighted(bnf_handle* h, const float* means, const float* scales, const double* weights,
                                          int64_t n_members, int64_t n_rows, const float* q, int32_t n_q,
                                          int32_t approximate, float* out);
int bnf_count_mixture_quantiles_weighted(bnf_handle* h, const float* loc, const float* aux, const double* weights,
                                         int64_t n_members, int64_t n_rows, const float* q, int32_t n_q, float* means,
                                         float* out);
int bnf_predictive_scores_weighted(bnf_handle* h, const float* loc, const float* aux, const double* weights,
                                   int64_t n_members, int64_t n_rows, const float* y, void* work, size_t work_bytes,
                                   float* lpd, float* pit, float* crps);
int bnf_count_rps_weighted(bnf_handle* h, const float* loc, const float* aux, const double* weights, int64_t n_members,
                           int64_t n_rows, const float* y, float* rps);

/* The matrix of per-member LOG DENSITIES of held-out observations: out DEVICE (n_members, n_rows) f32,
 * out[m][r] = log p_m(y_r), the f32 terms whose sums over r bnf_predictive_scores reports as member_ll (the forms of the
 * training loss, bnf_scoring.h).  loc, aux, y as for bnf_predictive_scores.  Every member of a row whose y is NaN or
 * infinite gets NaN; -inf is a legal value (a density of 0).  Runs on the handle's stream, does not touch the training
 * state, works on forward-only handles. */
int bnf_member_log_density(bnf_handle* h, const float* loc, const float* aux, int64_t n_members, int64_t n_rows,
                           const float* y, float* out);

/* STACKING of predictive distributions (Yao et al. 2018): simplex weights w over the members that maximise the held-out
 * log score f(w) = (1 / n) sum_r log sum_m w_m exp(logdens[m][r]), by EM on the mixture weights:
 *   g_m = (1 / n) sum_r exp(logdens[m][r] - lse_r),  lse_r = log sum_m w_m exp(logdens[m][r]),  w_m <- w_m g_m
 * (renormalised), which never lowers f.  f is concave and g its gradient, so gap = max_m g_m - 1 >= f(w*) - f(w) for the
 * optimum w*: the loop stops as soon as gap <= tol, or after max_iter updates, and reports the gap it stopped at -- a
 * bound on the distance to the optimum that needs no reference optimiser.
 *   logdens DEVICE (n_members, n_rows) f32 as bnf_member_log_density writes it.  A row holding a NaN is left out (not
 *     scored, not counted).  A row without a NaN is SCORED when lse_r is finite and DROPPED otherwise (every member with
 *     w_m > 0 at -inf): dropped rows are left out of every sum and counted.  n = the scored rows.
 *   w_init DEVICE (n_members,) f64 the starting weights, or NULL = uniform.  A weight of 0 stays 0.
 *   max_iter = 0: a pure evaluation of w_init (weights learned on one table scored on another).
 *   weights DEVICE (n_members,) f64: the result; for max_iter = 0 the bits of w_init.
 *   lpd DEVICE (n_rows,) f32 or NULL: (float) lse_r at the returned weights; NaN rows NaN, dropped rows -inf.
 *   info DEVICE (5,) f64, all evaluated at the weights that are returned: [0] f, [1] f at the starting weights, [2] gap,
 *     [3] updates done, [4] rows dropped.  Converged: info[2] <= tol.  No scored row: weights = the starting weights,
 *     [0], [1], [2] NaN, [3] = 0.
 *   work DEVICE, work_bytes: 8 * (BNF_STACK_STATE_DOUBLES + (n_members + 3) * ceil(n_rows / BNF_STACK_ROW_TILE)) bytes
 *     (the stop flag, the per-tile sums of every member, of lse and of the row counts); BNF_ERR_INVALID below that, and
 *     for n_members < 1, n_rows < 1, max_iter < 0, tol negative or NaN.
 * Everything after logdens is f64, exp and log included; every sum is in an order the shapes fix (no floating-point
 * atomics): two calls give the same bits.  An iteration is two kernels; they are enqueued BNF_STACK_BATCH iterations at a
 * time and return at once when the stop flag is set.  The call SYNCHRONISES on the handle's stream once per batch to read
 * that flag (beside bnf_profile_read the one entry point that waits for the device).  Runs
 * on the handle's stream, does not touch the training state, works on forward-only handles; the observation model of the
 * handle plays no part. */
#define BNF_STACK_ROW_TILE 1024
#define BNF_STACK_STATE_DOUBLES 8
#define BNF_STACK_BATCH 64
int bnf_stacking_weights(bnf_handle* h, const float* logdens, int64_t n_members, int64_t n_rows, const double* w_init,
                         int64_t max_iter, double tol, void* work, size_t work_bytes, double* weights, float* lpd,
                         double* info);

/* VALIDATION ON HELD-OUT ROWS DURING A FIT: one check.  Between two segments of bnf_train the caller scores the held-out
 * rows -- bnf_forward on a forward-only handle whose theta IS the training handle's parameter buffer, then
 * bnf_predictive_scores' member_ll -- and this call records every member's mean held-out log density and keeps a snapshot
 * of the member's parameters where the check is its best so far.  The decision is taken and the snapshot kept on the
 * device: a fit with checks has no more host round trips than one without.  The reference has no counterpart (its
 * ensemble_map runs num_epochs and returns the last parameters, inference.py:577-619).
 *   h            a bound MAP / MLE TRAINING handle: its members (cfg.members) and bound parameters (members, P) f32
 *   member_ll    DEVICE (members,) f64 as bnf_predictive_scores writes it for the held-out rows
 *   n_scored     the held-out rows with a finite target, >= 1 (the host knows it)
 *   epoch        epochs completed so far, recorded with the snapshot
 *   check, n_checks   index of this check and the number of checks of the fit: 0 <= check < n_checks
 *   curve        DEVICE (members, n_checks) f64 row-major: column `check` is written
 *   best_score   DEVICE (members,) f64 in/out     best_epoch DEVICE (members,) int64 in/out
 *   keep         DEVICE (members,) int32 out: 1 where this check became the member's best, else 0
 *   best_params  DEVICE (members, P) f32 in/out: the snapshots; must not overlap the handle's parameters
 * SCORE: score_m = member_ll[m] / (double)n_scored, one f64 division; curve[m][check] = score_m.
 * RULE: at check == 0, keep[m] = 1 always: whatever the score is, NaN or -inf included, it initialises best_score,
 *   best_epoch and best_params, so none of them is ever read uninitialised.  At check > 0,
 *   keep[m] = score_m > best_score[m] || (isnan(best_score[m]) && !isnan(score_m)): a tie keeps the earlier epoch, a NaN
 *   never replaces a number, -inf never replaces -inf.
 * SNAPSHOT: where keep[m] is set, best_score[m] = score_m, best_epoch[m] = epoch and row m of the handle's parameters is
 *   copied to row m of best_params, bit for bit.  Rows with keep[m] == 0 are not touched.
 * Two kernels (bnf_validation.h): the decision over the members, then the copy over (ceil(P / tile), members), which reads
 *   the finished decision.  No floating-point atomics: two calls give the same bits.
 * BNF_ERR_STATE for an unbound, a forward-only and a VI handle; BNF_ERR_INVALID for a NULL pointer, n_scored < 1,
 *   n_checks < 1, check outside [0, n_checks) and a best_params that overlaps the parameters; nothing is launched then.
 * Runs on the handle's stream and does not synchronise; reads the training parameters, writes none of the training state. */
int bnf_validation_check(bnf_handle* h, const double* member_ll, int64_t n_scored, int64_t epoch, int32_t check,
                         int32_t n_checks, double* curve, double* best_score, int64_t* best_epoch, int32_t* keep,
                         float* best_params);

/* SUMMARIES of an ensemble of sample paths, column by column: x DEVICE (n_samples, n_cols) f64 row-major -- the layout
 * bnf_predictive_group_sums writes, one column per group total -- and optionally the observed totals y DEVICE (n_cols,)
 * f64.  What a user of the totals would otherwise compute on the host from the whole matrix (np.quantile, an O(S^2) loop
 * per group for the CRPS).  Every column is sorted in LDS (bnf_totals.h); outputs, each skipped when its pointer is NULL:
 *   mean DEVICE (n_cols,) f64
 *   quant DEVICE (n_q, n_cols) f64: the levels q, a HOST array of n_q doubles in [0, 1], by numpy's default ('linear') rule:
 *     h = (n_samples - 1) q_j in f64, x_(floor h) + (h - floor h) (x_(floor h + 1) - x_(floor h)), exactly x_(h) when h is an
 *     integer.  n_q <= BNF_SUMMARY_MAX_QUANTILES per call (the levels travel as a kernel argument); required for n_q > 0
 *   pit DEVICE (2, n_cols) f64: [0] = #{x_s <= y_c} / n_samples, [1] = #{x_s < y_c} / n_samples
 *   crps DEVICE (n_cols,) f64: the ensemble CRPS E|X - y| - E|X - X'| / 2 as a V-statistic,
 *     (1 / S) sum_s |x_s - y_c| - (1 / S^2) sum_{i = 1..S} (2 i - S - 1) x_(i), evaluated on x - y_c
 * A column whose y_c is NaN or infinite gives NaN in crps and pit (mean and quant are still produced); a column that holds
 * a NaN sample gives NaN in every output.  y == NULL: a pure summary, crps and pit must be NULL too (BNF_ERR_INVALID).
 * n_samples <= BNF_SUMMARY_MAX_SAMPLES (a sorted column is 128 KiB of the CU's 160 KiB of LDS; a multi-pass sort is out
 * of scope); BNF_ERR_INVALID above that, for n_samples < 1, n_cols < 1, n_q < 0 and for a level outside [0, 1].
 * Everything is f64, every sum in an order the shapes fix: no atomics, two calls give the same bits.  No work buffer.
 * Runs on the handle's stream, does not touch the training state, works on forward-only handles; the observation model of
 * the handle plays no part. */
#define BNF_SUMMARY_MAX_SAMPLES 16384
#define BNF_SUMMARY_MAX_QUANTILES 64
int bnf_sample_summaries(bnf_handle* h, const double* x, int64_t n_samples, int64_t n_cols, const double* y,
                         const double* q, int32_t n_q, double* mean, double* quant, double* crps, double* pit);

/* The ENERGY SCORE of the joint sample paths against the observed vector, one number per call:
 *   out[0] = (1 / S) sum_s |X_s - y|_2 - (1 / (2 S^2)) sum_{s,t} |X_s - X_t|_2,   X_s = row s of x, S = n_samples
 * x, y as for bnf_sample_summaries (y required); out DEVICE (1,) f64.  The norms run over the columns whose y_c is finite,
 * the others are skipped in both terms; no finite y_c at all gives NaN.  Every distance is formed from direct differences
 * in f64; the cost is n_samples^2 n_cols / 2 differences (the pairs s < t, doubled).
 *   work DEVICE, work_bytes: one |X_s - y| per path and one partial sum per 64 x 64 tile of pairs on or above the diagonal,
 *     8 * (n_samples + T (T + 1) / 2) bytes, T = ceil(n_samples / BNF_ENERGY_SAMPLE_TILE); BNF_ERR_INVALID below that
 * n_samples <= BNF_SUMMARY_MAX_SAMPLES; BNF_ERR_INVALID above that and for n_samples < 1 or n_cols < 1.  The partial sums
 * are added in index order: no atomics, two calls give the same bits.  Runs on the handle's stream, does not touch the
 * training state, works on forward-only handles. */
#define BNF_ENERGY_SAMPLE_TILE 64
int bnf_sample_energy_score(bnf_handle* h, const double* x, int64_t n_samples, int64_t n_cols, const double* y,
                            void* work, size_t work_bytes, double* out);

/* The DEPENDENCE between the columns of the joint sample paths: their predictive covariance, their variogram, and the
 * variogram score of order p (Scheuerer & Hamill 2015) against the observed vector -- the companion of the energy score,
 * which is nearly blind to a wrong correlation structure.  x as for bnf_sample_summaries, S = n_samples, G = n_cols.
 *   mean DEVICE (G,) f64: m_c = (1 / S) sum_s x_sc
 *   cov DEVICE (G, G) f64: cov[i][j] = (1 / S) sum_s (x_si - m_i) (x_sj - m_j), from centred products (a total of 1e9 with
 *     a spread of 10 loses nothing); the divisor is S, the ensemble's own moment: np.cov(x.T, bias=True).  Needs mean.
 *   vario DEVICE (G, G) f64: vario[i][j] = (1 / S) sum_s |x_si - x_sj|^p
 *   score DEVICE (1,) f64: sum over the pairs i < j with y_i and y_j finite of w_ij (|y_i - y_j|^p - vario[i][j])^2, with
 *     y DEVICE (G,) f64 the observed totals and w_ij = 1, or pair_w[i][j] from pair_w DEVICE (G, G) f64 (read above the
 *     diagonal only; not validated: reading it would cost a sync).  Fewer than two finite y_c: NaN.
 *   p is 0.5, 1 or 2, compiled as sqrt(fabs d), fabs d and d * d; any other p is BNF_ERR_INVALID.
 * y, pair_w, mean, cov, vario and score may each be NULL: a NULL output is skipped, and with cov and vario NULL nothing of
 * size G^2 is written.  score needs y (BNF_ERR_INVALID without) and
 *   work DEVICE, work_bytes: one partial sum per BNF_PAIR_COL_TILE x BNF_PAIR_COL_TILE tile of pairs on or above the
 *     diagonal, 8 * T (T + 1) / 2 bytes, T = ceil(G / BNF_PAIR_COL_TILE); BNF_ERR_INVALID below that.  Not read otherwise.
 * Both matrices are written whole and are bitwise symmetric; vario[i][i] and the cell of two identical columns are exactly
 * 0.  A cell's bits depend on S and on its two columns only, not on G or on the other columns of the call: every cell is
 * one sequential sum over the paths (which stream through LDS BNF_PAIR_PATH_CHUNK at a time).  A column holding a NaN
 * sample is NaN in its row and column of both matrices, and makes the score NaN when its y_c is finite (whatever its
 * weights: w_ij is a plain factor).  The cost is S G^2 / 2 pair terms.  cov, vario or pair_w with
 * G > BNF_PAIR_MATRIX_MAX_COLS (a matrix of 128 MiB), n_samples < 1 and n_cols < 1 are BNF_ERR_INVALID; there is no cap on
 * n_samples (nothing is sorted).  Everything is f64, every sum in an order the shapes fix: no atomics, two calls give the
 * same bits.  Runs on the handle's stream, does not touch the training state, works on forward-only handles; the
 * observation model of the handle plays no part. */
#define BNF_PAIR_COL_TILE 64
#define BNF_PAIR_PATH_CHUNK 32
#define BNF_PAIR_MATRIX_MAX_COLS 4096
int bnf_sample_pair_moments(bnf_handle* h, const double* x, int64_t n_samples, int64_t n_cols, double p, const double* y,
                            const double* pair_w, double* mean, double* cov, double* vario, void* work, size_t work_bytes,
                            double* score);

/* A few representative SCENARIOS out of the joint sample paths: whole paths of the ensemble, each with a probability, and
 * what the ensemble loses by them -- fast forward selection (Heitsch & Roemisch 2003), which greedily picks the paths that
 * minimise the Kantorovich (Wasserstein-1) distance between the S equally likely paths and the chosen ones with optimally
 * redistributed mass.  x as for bnf_sample_summaries, S = n_samples, C = n_cols.
 * bnf_sample_distances: dist DEVICE (S, S) f64, the pairwise distances of the paths.  A column takes part when y is NULL or
 *   y_c is finite (the rule of bnf_sample_energy_score).  The term of column c for the pair (s, t) is d = x_sc - x_tc, and
 *   with scale DEVICE (C,) f64 d / scale_c: one IEEE division of the DIFFERENCE (a total of 1e9 with a spread of 10 loses
 *   nothing; the error of a term is relative to the term).  scale is not validated (reading it would cost a sync): a bad
 *   scale gives meaningless distances, never an access outside x / scale.
 *     p = 1: dist[s][t] = sum_c |term_c|          p = 2: dist[s][t] = sqrt(sum_c term_c * term_c)
 *   the sum over the participating columns in ascending order, ONE sequential f64 sum per cell, a product never contracted
 *   into the addition that follows: a cell's bits depend on its two paths and the participating columns only, not on S,
 *   the other paths or the tile geometry.  The matrix is written whole; dist[s][t] and dist[t][s] have the same bits; the
 *   diagonal is computed like any other cell: +0.0, or NaN for a path that holds a NaN in a participating column (such a
 *   path is NaN in its whole row and column).  No participating column: every cell is +0.0.
 *   ydist DEVICE (S,) f64: the same distance between path s and y DEVICE (C,) f64, the same sum; y and ydist are NULL
 *   together (BNF_ERR_INVALID otherwise).  n_samples <= BNF_SCENARIO_MAX_SAMPLES (a matrix of 128 MiB, the size
 *   BNF_PAIR_MATRIX_MAX_COLS allows); BNF_ERR_INVALID with nothing launched above that, for n_samples < 1, n_cols < 1, p
 *   outside {1, 2} and a NULL x or dist.  No work buffer.  S^2 C / 2 differences in 64 x 64 tiles of pairs on and above the
 *   diagonal, the mirrored tile stored through LDS in whole rows.
 * bnf_scenario_select: forward selection on a SYMMETRIC dist DEVICE (S, S) f64 (read by rows).  With dmin^0_s = +inf, for
 *   step i = 1 .. k:
 *     z_i(u) = sum_s min(dmin^(i-1)_s, dist[s][u])   for every path u not yet chosen
 *     chosen[i - 1] = u_i, the u with the smallest z_i, the LOWEST INDEX among equal ones
 *     dmin^i_s = min(dmin^(i-1)_s, dist[s][u_i])
 *     objective[i - 1] = z_i(u_i) / (double)S: the very sum that won, divided once -- the Kantorovich distance between
 *       the ensemble and the first i scenarios; nonincreasing in i
 *   and after step k
 *     assign DEVICE (S,) int32 or NULL: the smallest j in 0 .. k - 1 with dist[s][chosen[j]] == dmin^k_s (among equally
 *       near scenarios the earliest chosen)       nearest DEVICE (S,) f64 or NULL: dmin^k_s
 *     prob DEVICE (k,) f64: #{s : assign[s] = j} / (double)S
 *   Identical paths have distance 0 (totals of counts repeat all the time): once every distinct path is chosen all
 *   remaining candidates tie, and the lowest unchosen index is taken with probability 0.  That is defined, not an error.
 *   ydist DEVICE (S,) f64 or NULL, as bnf_sample_distances writes it; with it (obs_nearest and obs are required then, and
 *   ignored without):
 *     obs_nearest DEVICE (1,) int32: the earliest chosen j that minimises ydist[chosen[j]]       obs DEVICE (3,) f64:
 *     obs[0] that distance; obs[1] = #{s : nearest_s <= obs[0]} / S; obs[2] = #{s : nearest_s < obs[0]} / S -- the PIT of the
 *     observed vector's distance to the scenario set among the paths' own (near 1: the observed lies farther from every
 *     scenario than nearly every path of the forecast does)
 *   A NaN cell anywhere in dist: chosen, assign and obs_nearest are -1 everywhere and objective, prob, nearest and obs NaN
 *   (a first kernel sets a device flag the later ones read; the host never waits for it).
 *   The sum z_i(u) over s is in an order S alone fixes: with 256 threads, thread t adds s = t, t + 256, ... in that order,
 *   then the wave butterfly (v += shfl_xor(v, off), off = 32 .. 1), then the four waves in order.  All k steps are
 *   enqueued back to back; the pick of a step stays on the device.  S^2 reads of dist per step.
 *   work DEVICE, work_bytes: dmin and z (S f64 each), the taken marks (S int32), the flag and the pick:
 *     20 * n_samples + 16 bytes, 8-byte aligned; BNF_ERR_INVALID below that
 *   1 <= k <= n_samples <= BNF_SCENARIO_MAX_SAMPLES; BNF_ERR_INVALID otherwise and for a NULL dist, work, chosen, objective
 *   or prob, with nothing launched.
 * Both: everything is f64, no floating-point atomics, two calls give the same bits; they run on the handle's stream, do not
 * touch the training state, work on forward-only handles; the observation model of the handle plays no part. */
#define BNF_SCENARIO_MAX_SAMPLES 4096
int bnf_sample_distances(bnf_handle* h, const double* x, int64_t n_samples, int64_t n_cols, const double* scale,
                         const double* y, int32_t p, double* dist, double* ydist);
int bnf_scenario_select(bnf_handle* h, const double* dist, int64_t n_samples, int32_t k, const double* ydist, void* work,
                        size_t work_bytes, int32_t* chosen, double* objective, double* prob, int32_t* assign,
                        double* nearest, int32_t* obs_nearest, double* obs);

/* How the columns of the joint sample paths RANK against each other within a path -- "which groups are among the k
 * largest" -- which no marginal shows.  x as for bnf_sample_summaries, S = n_samples, G = n_cols.
 * bnf_sample_ranks: per path s the ranked values are v_sg = x_sg / scale_g, a plain IEEE f64 division, with
 *   scale DEVICE (G,) f64 a per-column divisor (a population: rank per capita), or NULL: v = x.  Not validated (reading it
 *     would cost a sync): a bad scale gives meaningless ranks, never an access outside x / scale.
 *   out_above DEVICE (S, G) int32: #{h : v_sh > v_sg}
 *   out_ties DEVICE (S, G) int32: #{h : v_sh == v_sg}, which counts g itself: >= 1
 *   out_rank DEVICE (S, G) f64: the mid-rank above + (ties + 1) / 2, a multiple of 0.5 -- rank 1 is the LARGEST value; the
 *     matrix bnf_sample_summaries takes (mean rank, rank quantiles, CRPS / PIT against the observed ranks)
 * Tied columns share their block of ranks equally and are never told apart by their index (totals of counts tie all the
 * time).  The comparison is a total order: -0.0 and +0.0 tie, +inf values tie, NaNs tie with each other, and a NaN ranks
 * below everything, -inf included; so the integers depend on the path's values alone, and sum_g rank_sg = G (G + 1) / 2.
 * Each output is skipped when NULL; all three NULL is BNF_ERR_INVALID.  One workgroup sorts the G keys of a path in LDS
 * (8 bytes each, padded to a power of two: G <= BNF_RANK_MAX_COLS, BNF_ERR_INVALID beyond) and every column finds its block
 * by two binary searches: G log^2 G per path.  n_samples < 1 and n_cols < 1 are BNF_ERR_INVALID; there is no cap on
 * n_samples.  The observed ranks are this call on the observed totals as a 1 x G matrix.
 * bnf_rank_probabilities: out DEVICE (top_k, G) f64,
 *   out[k - 1][g] = (1 / S) sum_s [above_sg < k <= above_sg + ties_sg] / ties_sg,   k = 1 .. top_k:
 * the probability that column g takes rank slot k, a tied block handing each of its slots out in equal shares.  Every row
 * k <= G sums to 1 over the columns (a slot is handed out once per path); with top_k = G every column sums to 1.  Every
 * cell is one sequential f64 sum over the paths in path order (which stream through LDS BNF_RANK_PATH_CHUNK at a time),
 * then divided by (double)S: its bits depend on S and on that column's above / ties only.  1 <= top_k <= n_cols and
 * top_k * n_cols <= BNF_RANK_MAX_CELLS, BNF_ERR_INVALID otherwise.  above / ties are not validated.
 * Both: no floating-point atomics, two calls give the same bits; they run on the handle's stream, do not touch the
 * training state, work on forward-only handles; the observation model of the handle plays no part. */
#define BNF_RANK_MAX_COLS 16384          /* one path's values sorted in LDS */
#define BNF_RANK_PATH_CHUNK 32           /* paths per LDS chunk of bnf_rank_probabilities */
#define BNF_RANK_MAX_CELLS (1 << 24)     /* top_k * n_cols of bnf_rank_probabilities: 128 MiB */
int bnf_sample_ranks(bnf_handle* h, const double* x, int64_t n_samples, int64_t n_cols, const double* scale,
                     double* out_rank, int32_t* out_above, int32_t* out_ties);
int bnf_rank_probabilities(bnf_handle* h, const int32_t* above, const int32_t* ties, int64_t n_samples, int64_t n_cols,
                           int32_t top_k, double* out);

/* SIMULTANEOUS BANDS of the joint sample paths: bands that hold a whole path with a given probability, where the quantiles
 * of bnf_sample_summaries hold each column alone -- the rank envelope of Myllymaki et al. 2017 ("Global envelope tests").
 * x as for bnf_sample_summaries, S = n_samples, C = n_cols (a column is a table row, or a position of a running-total
 * curve); col_group DEVICE (C,) int32 the group of every column, an entry outside [0, G) = the column takes no part;
 * G = n_groups.  Comparisons use the total order of bnf_sample_ranks: -0.0 == +0.0, infinities of one sign tie.
 *   depth of path s at column c   d_sc = min(#{t : x_tc <= x_sc}, #{t : x_tc >= x_sc}) - 1, in [0, S - 1] (s counts itself);
 *                                 in a column that holds a NaN sample every path has depth -1
 *   depth of path s in group g    D_sg = min of d_sc over the columns of g
 *   band k at a column            [x_(k), x_(S-1-k)] of the column sorted ascending, 0-indexed; path s lies inside band k at
 *                                 every column of g exactly when D_sg >= k
 * Everything is an integer, a value picked from x, or ONE f64 division of a count by (double)S.
 * bnf_sample_depths: lowers depth DEVICE (S, G) int32 to min(depth, D) with integer atomicMin only; the CALLER fills it
 *   with BNF_DEPTH_NONE first, so several calls -- over chunks of columns, or over several curves of the same paths --
 *   accumulate into one joint depth, in any order.  A group no column of the call belongs to is not touched.
 *   y DEVICE (C,) f64 observed values, or NULL: obs_depth DEVICE (G,) int32, pre-filled the same way, is lowered to
 *     OD_g = min over the columns of g whose y_c is not NaN of od_c = min(#{t : x_tc <= y_c}, #{t : x_tc >= y_c}) - 1,
 *     in [-1, S - 1]: -1 = outside the envelope of all paths at some column (and in a column with a NaN sample); y lies
 *     inside band k of g exactly when OD_g >= k.  y and obs_depth are NULL together (BNF_ERR_INVALID otherwise).
 *   One workgroup sorts a slab of up to 8 adjacent columns in LDS (the layout of bnf_sample_summaries, 8 bytes a key,
 *   padded to a power of two with a key above every real one) and every (path, column) finds its tie block by two binary
 *   searches over the real cells only: C S log^2 S / 2 compare-exchanges, 2 C S log S probes.
 * bnf_depth_levels: from depth (and obs_depth, or NULL) as bnf_sample_depths left them, with ge_g(k) = #{s : D_sg >= k}:
 *   need HOST n_cov int32 in [1, S]: for a coverage c, ceil(c S) (the caller rounds); k_query HOST n_query int32, any value;
 *     both travel as kernel arguments: n_cov, n_query <= BNF_BAND_MAX_LEVELS
 *   level DEVICE (n_cov, G) int32: k* = the largest k with ge_g(k) >= need_i -- the need_i-th largest of D[:, g], in [-1, S - 1]
 *   achieved DEVICE (n_cov, G) f64: ge_g(k*) / S >= need_i / S, the share of the paths that band k* holds whole
 *   joint DEVICE (n_query, G) f64: ge_g(k_query_i) / S -- e.g. with k = floor((S - need) / 2), the pointwise band that holds
 *     need samples at each column, the share of the paths that band holds WHOLE
 *   obs_pit DEVICE (2, G) f64: [0] = #{s : D_sg <= OD_g} / S, [1] = #{s : D_sg < OD_g} / S: the depth PIT of the observed
 *     curve (a value drawn uniformly between the two is uniform when y is exchangeable with the paths; small = the observed
 *     curve is more extreme than nearly every path).  NaN where OD_g is outside [-1, S - 1] (no observed column).  Needs
 *     obs_depth
 *   Each output is skipped when NULL.  A group with a depth outside [-1, S - 1] is EMPTY (BNF_DEPTH_NONE: no column took
 *   part; or the input is not ours): level -1 and NaN ratios; such a value never indexes anything.  A group poisoned by a
 *   NaN column (every depth -1) has level -1 and achieved 1.  One workgroup per group: a histogram of D + 1 over S + 1 bins
 *   in LDS (integer atomics), a suffix scan, then every output is a lookup: S + G reads of depth, no sort.
 * bnf_sample_envelope: the bands themselves.  level DEVICE (n_levels, G) int32 as bnf_depth_levels writes it (or any k);
 *   lower, upper DEVICE (n_levels, C) f64: lower[j][c] = x_(k), upper[j][c] = x_(S-1-k) with k = level[j][group of c]; NaN
 *   for k outside [0, S - 1], for a column that takes no part and for one that holds a NaN sample.  A picked -0.0 comes
 *   back as +0.0.  The same slab sort, then picks.  1 <= n_levels <= BNF_BAND_MAX_LEVELS.
 * All three: BNF_ERR_INVALID with nothing launched for a NULL required pointer, n_samples, n_cols or n_groups < 1,
 * n_samples > BNF_SUMMARY_MAX_SAMPLES, a need outside [1, n_samples] and more levels than BNF_BAND_MAX_LEVELS.  No
 * floating-point atomics, two calls give the same bits; they run on the handle's stream, do not touch the training state,
 * work on forward-only handles; the observation model of the handle plays no part. */
#define BNF_DEPTH_NONE 0x7fffffff        /* the pre-fill of depth and obs_depth: no column has been seen */
#define BNF_BAND_MAX_LEVELS 64           /* coverage levels / queried bands per call */
int bnf_sample_depths(bnf_handle* h, const double* x, int64_t n_samples, int64_t n_cols, const int32_t* col_group,
                      int64_t n_groups, const double* y, int32_t* depth, int32_t* obs_depth);
int bnf_depth_levels(bnf_handle* h, const int32_t* depth, int64_t n_samples, int64_t n_groups, const int32_t* need,
                     int32_t n_cov, const int32_t* k_query, int32_t n_query, const int32_t* obs_depth, int32_t* level,
                     double* achieved, double* joint, double* obs_pit);
int bnf_sample_envelope(bnf_handle* h, const double* x, int64_t n_samples, int64_t n_cols, const int32_t* col_group,
                        const int32_t* level, int32_t n_levels, int64_t n_groups, double* lower, double* upper);

/* ---- introspection used by tests and bench.py ------------------------------ */
/* One forward+backward of every local member on batch `step` of `epoch` WITHOUT
 * the optimiser update: grads DEVICE (members*S, P) f32 receives d(step loss)/d
 * theta of the likelihood part + prior part exactly as Adam would consume it;
 * loss DEVICE (members*S,) f32 the step loss.  theta_eff may be NULL (use the
 * bound params; VI: the z samples of that step). */
int bnf_debug_loss_and_grad(bnf_handle* h, int64_t epoch, int64_t step,
                            float* grads, float* loss);
/* Row ids the engine uses for (epoch, step): out DEVICE (members, B) int32
 * (MAP: per-member shuffle, inference.py:593-597; VI: one shared batch,
 * :704-709; full batch: 0..N-1). */
int bnf_debug_row_index(bnf_handle* h, int64_t epoch, int64_t step, int32_t* out);
/* VI noise of a step: out DEVICE (members, S, P) f32. */
int bnf_debug_vi_eps(bnf_handle* h, int64_t step, float* out);
/* Verification hook: from now on every VI step takes its reparameterisation noise from `eps`
 * (DEVICE, (members, S, P) f32 standard normals, caller-owned, read at each step; NULL = the
 * engine's own counter-based generator again).  It lets a test feed the noise of
 * tfp.vi.fit_surrogate_posterior_stateless (inference.py:727-738) and compare with the reference's
 * golden predictions element-wise; not meant for production sizes. */
int bnf_debug_vi_noise(bnf_handle* h, const float* eps);
/* Copy of an internal activation buffer, as f32: what = 0 features H0 (E',B,F),
 * 1+l hidden output H_{l+1} (E',B,W) for l < depth-1 (the last hidden output is
 * never stored), 100+l pre-activation A_l (E',B,W), 200 network output (E',B),
 * 300+l dZ_l (E',B,W), 400 dH0 (E',B,F). Valid after bnf_debug_loss_and_grad. */
int bnf_debug_activation(bnf_handle* h, int32_t what, float* out);
/* Raw C = A * Bt^T of the dense-contraction core (A (M,K), Bt (N,K), K a multiple
 * of 64, dtype = handle dtype, inputs given as f32 and converted) -> C (M,N) f32. */
int bnf_debug_gemm_nt(bnf_handle* h, const float* A, const float* Bt, int32_t M,
                      int32_t N, int32_t K, float* C);

/* Raw C = A^T * B of the weight-gradient core on row-major operands (A (R,M), B (R,N),
 * R a multiple of 64, M and N multiples of 8; inputs f32, converted to the handle dtype)
 * -> C (M,N) f32. */
int bnf_debug_gemm_tn(bnf_handle* h, const float* A, const float* B, int32_t R, int32_t M,
                      int32_t N, float* C);

/* Test hook: fills all 160 KiB of LDS of every CU with `pattern`-derived garbage (NaN bit patterns
 * for pattern = 0x7fc00000).  LDS is not cleared between kernels: a kernel that reads LDS it has not
 * written sees whatever the previous kernel left there, so parity tests run with poisoned LDS. */
int bnf_debug_poison_lds(bnf_handle* h, uint32_t pattern);

/* Per-kernel HIP-event timing on the handle's stream.  kernel = "*" brackets
 * every launch with an event pair, a kernel name (as reported by
 * bnf_profile_read, e.g. "gemm_fwd") only that kernel, NULL switches it off.
 * Enable, run bnf_train, then read (read synchronises on the recorded events).
 * names/avg_ms/calls: arrays of length *n (in: capacity, out: used). */
int bnf_profile_enable(bnf_handle* h, const char* kernel);
int bnf_profile_read(bnf_handle* h, int32_t* n, const char** names, double* avg_ms,
                     int64_t* calls);
/* Algorithmic FLOPs of one launch of kernel `name` for the bound configuration
 * (DESIGN.md section 4), 0 for non-contraction kernels. */
double bnf_kernel_flops(const bnf_handle* h, const char* name);

/* ---- the job's one data collective: the posterior gather -----------------------------------
 * Replaces what `jax.pmap` does implicitly when the reference's fit / predict return
 * (/root/reference/src/bayesnf/inference.py:452 `np.array(params_i)`, :486-492 the per-device
 * predictive means concatenated on the default device): every rank contributes its members'
 * device-resident parameters / predictive means and receives everyone's.  One RCCL all-gather
 * over xGMI; librccl.so is dlopen'ed on first use (the engine itself has no link dependency).
 *   id       BNF_COMM_ID_BYTES bytes made by rank 0 (bnf_comm_unique_id) and handed to every
 *            rank by the host (any side channel: the Python layer broadcasts it)
 *   send     DEVICE, bytes_per_rank bytes;  recv DEVICE, world * bytes_per_rank bytes, rank-major
 *   stream   hipStream_t the collective is enqueued on (no host synchronisation) */
#define BNF_COMM_ID_BYTES 128
typedef struct bnf_comm bnf_comm;
int bnf_comm_available(void);   /* 0 when librccl.so and its symbols resolve (local, cheap: no id, no listener) */
int bnf_comm_unique_id(void* id);
int bnf_comm_create(const void* id, int32_t world, int32_t rank, int32_t device, bnf_comm** out);
int bnf_allgather(bnf_comm* c, const void* send, void* recv, size_t bytes_per_rank, void* stream);
/* ONE process driving n devices -- the reference's own shape (`jax.pmap` over `jax.local_devices()`,
 * inference.py:573-579,445): `bnf_comm_create_local` makes one communicator per listed device in one call
 * (ncclCommInitAll; out[n]; a device listed twice is refused), `bnf_allgather_group` enqueues every local rank's
 * all-gather in one group (send[i] / recv[i] / streams[i] on comms[i]'s device; recv[i] receives all n blocks;
 * `comms` must be the WHOLE set of one bnf_comm_create_local call in rank order -- checked, BNF_ERR_INVALID
 * otherwise: a partial set would leave ncclGroupEnd waiting; streams == NULL or a NULL entry = the default stream).
 * `bnf_comm_available` already requires the group symbols, so callers agree on the full capability up front. */
int bnf_comm_create_local(int32_t n, const int32_t* devices, bnf_comm** out);
int bnf_allgather_group(int32_t n, bnf_comm* const* comms, const void* const* send, void* const* recv,
                        size_t bytes_per_rank, void* const* streams);
void bnf_comm_destroy(bnf_comm* c);

#ifdef __cplusplus
}
#endif
#endif /* BNF_H_ */
