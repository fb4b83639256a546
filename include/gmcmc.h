/*
 * gmcmc.h — C ABI of the MI355X many-chain HMC / NUTS / Metropolis-Hastings
 * engine (libgmcmc.so, HIP kernels for gfx950).
 *
 * This is the drop-in boundary for the hot path of SauersML/general-mcmc
 * (reference snapshot under /root/reference). Each entry point names the
 * reference interface it replaces. Plain pointers and sizes only; no torch
 * types. All functions return GM_OK (0) or an error code; the message of the
 * last error on the calling thread is available from gm_last_error(). No
 * function aborts the process: the reference's panics (shape asserts,
 * euclidean.rs:116-120/432-437, distributions.rs:267) become GM_EINVAL.
 *
 * Data layout conventions
 *   - host initial positions / host outputs are row-major, reference layout:
 *     init [n_chains][dim]           (hmc.rs:119-124, Vec<Vec<T>> flattened)
 *     samples [n_chains][n_collect][dim] (hmc.rs:179-180 stack+permute)
 *   - device-resident samples (gm_*_run_device) are [n_collect][n_chains][dim]
 *     (one contiguous [C,D] slab per collected step, as BatchedGenericHMC::
 *     run_positions returns one Tensor<B,2> per step, batched_hmc.rs:115-123).
 *   - element type is given by gm_dtype (f32 or f64) everywhere.
 *
 * Threading: one sampler must not be used from two threads at once
 * (&mut self in the reference, hmc.rs:164). Distinct samplers may run
 * concurrently; each owns a HIP stream on the device that was current
 * (gm_set_device) when it was created.
 */
#ifndef GMCMC_H
#define GMCMC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---------------------------------------------------- */
#define GM_OK 0
#define GM_EINVAL 1 /* bad argument / shape (reference: assert_eq!/expect panics) */
#define GM_EHIP 2   /* HIP runtime error */
#define GM_ENOMEM 3 /* device allocation failed */
#define GM_ERCCL 4  /* RCCL error */
#define GM_ESTATE 5 /* call not valid in the sampler's current state */

/* GM_DTYPE_INT_: not a dtype; it widens the enum's value range to int, so a
 * caller passing any other integer gets GM_EINVAL instead of undefined
 * behaviour in the C++ implementation (found by the UBSan host build). */
typedef enum gm_dtype { GM_F32 = 0, GM_F64 = 1, GM_DTYPE_INT_ = 0x7fffffff } gm_dtype;

/* ---- targets (replaces the user-implemented traits) ---------------------
 * BatchedGradientTarget::unnorm_logp_batch   distributions.rs:67-78
 * GradientTarget::unnorm_logp(+_and_grad)     distributions.rs:80-90
 * Target::unnorm_logp                         distributions.rs:107-110
 * Built-in targets get analytic gradients instead of burn autodiff
 * (hmc.rs:42-61).                                                          */
typedef enum gm_target_kind {
  GM_TARGET_ROSENBROCK = 1, /* RosenbrockND (a=1,b=100) distributions.rs:535-555;
                               Rosenbrock2D{a,b} distributions.rs:495-530    */
  GM_TARGET_ISO_GAUSS = 2,  /* IsotropicGaussian as Target, distributions.rs:398-406 */
  GM_TARGET_GAUSS = 3,      /* DiffableGaussian2D distributions.rs:215-320 generalised
                               to D dims: logp = norm_const - 0.5 (x-mu)^T P (x-mu),
                               P = Sigma^-1 supplied row-major; also Gaussian2D as a
                               Target (distributions.rs:193-207) with norm_const = 0 */
  GM_TARGET_CUSTOM = 4,     /* user code (the reference's Target / GradientTarget
                               traits, distributions.rs:67-110): HIP source defining
                                 template <class T> __device__
                                 T gm_logp_grad(const T* x, T* g, const T* params);
                               for one chain (x, g of length GM_DIM, a macro = dim),
                               compiled at run time (hiprtc) into the sampler kernels;
                               one chain per lane, dim <= 256 */
  GM_TARGET_GLM = 5         /* generalised linear model with canonical link and an
                               independent Gaussian prior, described by gm_glm_desc
                               (gm_target.glm); dim = number of columns, 1..128 */
} gm_target_kind;

/* GLM families (gm_glm_desc.family); eta_n = sum_j x[n][j] theta_j + offset_n */
#define GM_GLM_BERNOULLI_LOGIT 1 /* A(eta) = max(eta,0) + log1p(exp(-|eta|)), mu = logistic(eta); 0 <= y <= 1 */
#define GM_GLM_POISSON_LOG 2     /* A(eta) = mu(eta) = exp(eta); y >= 0; offset = log exposure */

/* GM_TARGET_GLM:
 *   logp  = sum_n ( y_n eta_n - A(eta_n) ) - 0.5 sum_j theta_j^2 / prior_sd_j^2
 *   grad_j = sum_n x[n][j] ( y_n - mu(eta_n) ) - theta_j / prior_sd_j^2
 * (additive constants that do not depend on theta are dropped; a non-finite
 * log-density is not clamped: the proposal is rejected / the tree divergent).
 * The arrays are host memory, copied to the device in the sampler's dtype when
 * a sampler (or gm_target_logp_grad) is created, and may be freed afterwards.
 * Creation returns GM_EINVAL, naming the first offending row or column, unless
 * every x, y, offset and prior_sd is finite, y is in the family's range,
 * prior_sd > 0, n_rows >= 1 and 1 <= dim <= 128.
 * Takes gm_target_logp_grad, gm_hmc_create (per-chain step sizes, diagonal
 * metric, their warm-up, statistics) and gm_nuts_create (identity or diagonal
 * adaptive metric, either convention, per chain). MH, the dense HMC metric,
 * the NUTS dense and pooled metrics, wide layouts and gm_bv_target_create
 * return GM_EINVAL ("GLM target: ..."). */
typedef struct gm_glm_desc {
  int32_t family;         /* GM_GLM_BERNOULLI_LOGIT or GM_GLM_POISSON_LOG */
  int32_t reserved;
  int64_t n_rows;
  const double* x;        /* [n_rows*dim] row-major design matrix */
  const double* y;        /* [n_rows] */
  const double* offset;   /* [n_rows] or NULL (all 0) */
  const double* prior_sd; /* [dim] */
} gm_glm_desc;

typedef struct gm_target {
  int32_t kind;          /* gm_target_kind */
  int32_t reserved;
  int64_t dim;           /* must equal the sampler's dim */
  double a, b;           /* ROSENBROCK: logp = -sum_i [ b (x_{i+1}-x_i^2)^2 + (a-x_i)^2 ] */
  double std;            /* ISO_GAUSS: logp = -0.5 * sum x^2 / std^2 */
  const double* mean;    /* GAUSS: [dim] */
  const double* prec;    /* GAUSS: [dim*dim] row-major inverse covariance */
  double norm_const;     /* GAUSS: additive constant */
  const char* source;    /* CUSTOM: HIP source of gm_logp_grad (copied) */
  const double* params;  /* CUSTOM: [n_params] copied to the device in the sampler dtype */
  int64_t n_params;      /* CUSTOM: passed to gm_logp_grad as `params` */
  /* Appended after the struct's first release. The library reads this field
   * only when kind == GM_TARGET_GLM, a kind that callers compiled against the
   * shorter struct cannot set knowingly: their gm_target objects keep
   * working unchanged. Callers that set GM_TARGET_GLM must be compiled
   * against this header. */
  const gm_glm_desc* glm; /* GLM: the model (copied at creation) */
} gm_target;

/* Compile a CUSTOM target's source for the sampler kernels without running it
 * (kind: 1 HMC, 2 MH, 3 NUTS, 4 HMC with per-chain step sizes / metric /
 * warm-up, 5 HMC with a dense metric (2 <= dim <= 64), 6 MH with per-chain
 * proposal scales / shape / warm-up,
 * 0 log-density/gradient); GM_EINVAL with the
 * compiler log in gm_last_error() when it does not compile. */
int gm_custom_target_check(const char* source, gm_dtype dtype, int64_t dim, int32_t kind);

/* DiffableGaussian2D::new (distributions.rs:229-253) generalised: from a mean
 * and covariance compute the precision matrix and norm_const =
 * -(dim ln(2 pi) + ln|Sigma|)/2. For dim == 2 the closed-form 2x2 inverse of
 * the reference is used bit-for-bit; otherwise a Cholesky factorisation. */
int gm_gauss_from_cov(int64_t dim, const double* cov, double* prec_out, double* norm_const_out);

/* Evaluate a target on host-provided points (device compute): logp [n],
 * grad [n][dim] (grad may be NULL). Replaces logp_and_grad
 * (batched_hmc.rs:18-22, hmc.rs:42-61). */
int gm_target_logp_grad(const gm_target* target, gm_dtype dtype, int64_t n, const void* x,
                        void* logp_out, void* grad_out);

/* Initial positions: n x dim iid N(0,1) from the engine's counter-based
 * stream keyed by `seed` (core.rs:434-475 init / init_det / init_with_seed
 * analogue: same distribution and row-by-row meaning, not the same numbers,
 * see gm_rng.h). Host-side; out is [n][dim] of dtype. */
int gm_init_positions(uint64_t seed, int64_t n, int64_t dim, gm_dtype dtype, void* out);
/* Rows [row0, row0 + n) of the same stream (a shard's block of a global
 * start: rank r of a sharded run takes rows [offset_r, offset_r + n_r)). */
int gm_init_positions_rows(uint64_t seed, int64_t row0, int64_t n, int64_t dim, gm_dtype dtype, void* out);

/* ---- device / errors ------------------------------------------------ */
const char* gm_last_error(void);

/* "src:<digest>": the digest of the sources this library was built from
 * (tools/source_digest.py over csrc/, this header and the Makefile); the
 * Python layer refuses a library whose digest differs from its tree's. */
const char* gm_build_info(void);
int gm_device_count(int* count);
/* Select the calling thread's device. Called before the device is first used,
 * it also makes the thread's host waits spin (hipDeviceScheduleSpin): run
 * completion is then seen microseconds sooner. */
int gm_set_device(int device);
int gm_device_synchronize(void);

/* ---- samplers ----------------------------------------------------------- */
typedef struct gm_sampler gm_sampler;

/* HMC::new (hmc.rs:113-134) / BatchedGenericHMC::new (batched_hmc.rs:62-84).
 * init: host [n_chains][dim] of dtype. chain_offset: global id of chain 0
 * (used to key the per-chain random streams; 0 unless chains are sharded
 * across processes/GPUs). */
int gm_hmc_create(const gm_target* target, gm_dtype dtype, int64_t n_chains, int64_t dim,
                  const void* init, double step_size, int64_t n_leapfrog,
                  int64_t chain_offset, gm_sampler** out);

/* ---- HMC warm-up: per-chain step sizes and a per-chain diagonal metric ----
 * No reference counterpart (the reference's HMC takes one step size and the
 * identity metric, hmc.rs:113-134). A sampler on which none of these calls
 * was made runs exactly as before. They need an HMC sampler (GM_ESTATE
 * otherwise) with dim <= 1024 (GM_EINVAL on a wide layout).
 *
 * With a metric M (diagonal, per chain) a transition draws p = sqrt(M) z from
 * the same momentum normals z, drifts with q += eps * M^-1 p and weighs the
 * kinetic energy 0.5 p' M^-1 p; with equal step sizes and M = I it returns
 * the bits of the plain path.
 *
 * gm_hmc_set_adaptation arms a warm-up: the n_discard transitions of the next
 * gm_run* call (a run with n_discard == 0 adapts nothing and stays armed)
 * adapt, per chain, the step size by dual averaging towards target_accept
 * (gamma .05, t0 10, kappa .75, as NUTS here) and, in mode 2, a diagonal
 * metric from the Welford variance of the positions in the windows of the
 * NUTS schedule (start_buffer, end_buffer, initial_window doubling up to 400;
 * at a window end with >= 5 positions: M^-1 = max((1 - regularize) var +
 * regularize, max(jitter, 1e-10)), statistics reset, dual averaging restarted
 * from eps_bar). After the last warm-up transition eps = eps_bar; later runs
 * and gm_step sample with the frozen step sizes and metric. Calling it again
 * re-arms. mode 0 drops all per-chain state: the sampler is back on the
 * creation step size, the identity metric and the plain path.
 * Metric convention: M^-1 is the regularised sample variance (Stan, PyMC);
 * the NUTS path follows the reference and stores 1/var in its `inv`.
 * GM_EINVAL unless 0 < target_accept < 1, the window sizes are >= 0 and
 * regularize is in [0, 1]. */
int gm_hmc_set_adaptation(gm_sampler* s, int32_t mode /* 0 off, 1 step size, 2 step size + diagonal metric */,
                          double target_accept, int64_t start_buffer, int64_t end_buffer,
                          int64_t initial_window, double regularize, double jitter);
/* Per-chain step sizes eps[n_chains] (finite, > 0; rounded to the sampler
 * dtype); eps_bar is set to the same values. */
int gm_hmc_set_step_sizes(gm_sampler* s, const double* eps);
/* Per-chain (eps, eps_bar), [n_chains] each, either may be NULL; the creation
 * step_size for every chain before any of these calls. */
int gm_hmc_get_step_sizes(gm_sampler* s, double* eps, double* eps_bar);
/* The metric as M^-1: diag_inv [n_chains][dim] of the sampler dtype, every
 * entry finite and > 0 (GM_EINVAL otherwise, the sampler unchanged);
 * sqrt(M) = 1/sqrt(diag_inv) is derived from it. */
int gm_hmc_set_metric(gm_sampler* s, const void* diag_inv);
/* M^-1 and sqrt(M), [n_chains][dim] of the sampler dtype, either may be NULL;
 * ones before any of these calls. */
int gm_hmc_get_metric(gm_sampler* s, void* diag_inv, void* diag_sqrt);

/* ---- HMC warm-up: one dense metric shared by all chains ---------------------
 * Stan's convention: M^-1 = Sigma, the regularised covariance of the warm-up
 * positions POOLED over all chains of the sampler (they target one
 * distribution). With Sigma = L L^T and A = L^-T a transition draws p = A z
 * from the same momentum normals z, drifts with q += eps * Sigma p and weighs
 * the kinetic energy 0.5 p' Sigma p; with Sigma = I it returns the bits of the
 * plain path. Step sizes stay per chain (gm_hmc_set_step_sizes /
 * gm_hmc_get_step_sizes work unchanged). A sampler on which none of these
 * calls was made runs exactly as before.
 * Shapes: an HMC sampler (GM_ESTATE otherwise) with 2 <= dim <= 64 at the
 * dim's default layout, next_pow2(dim) x 1 for a built-in target and 1 x dim
 * for a CUSTOM one, whose source is compiled into the kernel at the first of
 * these calls (GM_EINVAL otherwise; a dense-metric sampler refuses
 * gm_sampler_set_layout to another layout).
 *
 * gm_hmc_set_dense_adaptation arms the warm-up (the n_discard transitions of
 * the next gm_run* call, as gm_hmc_set_adaptation): per-chain dual averaging
 * of the step size and, in the windows of the same schedule, float64 pooled
 * statistics of every chain's position. At a window end with >= 5 transitions
 * collected: Sigma = (1 - regularize) S + regularize I (S the pooled sample
 * covariance), each diagonal entry floored at max(jitter, 1e-10), factored in
 * float64; a failed factorisation keeps the previous metric and is counted;
 * either way the statistics reset and the dual averaging restarts from
 * eps_bar. It drops any per-chain diagonal metric and keeps the step sizes and
 * a dense metric already set. Validation as gm_hmc_set_adaptation.
 * gm_hmc_set_adaptation drops the dense metric (every mode); gm_hmc_set_metric
 * and gm_hmc_get_metric return GM_ESTATE on a dense-metric sampler. */
int gm_hmc_set_dense_adaptation(gm_sampler* s, double target_accept, int64_t start_buffer, int64_t end_buffer,
                                int64_t initial_window, double regularize, double jitter);
/* M^-1 = minv [dim][dim], float64: finite, exactly symmetric and positive
 * definite (GM_EINVAL otherwise, the sampler unchanged). On a sampler without
 * a dense metric it also drops any per-chain diagonal metric and disarms a
 * warm-up armed by gm_hmc_set_adaptation (the step sizes stay); on a
 * dense-metric sampler an armed dense warm-up stays armed. */
int gm_hmc_set_dense_metric(gm_sampler* s, const double* minv);
/* minv = Sigma and a_factor = A = L^-T (upper triangular), [dim][dim] float64
 * row-major; the numbers of metric updates and of failed factorisations of the
 * warm-ups so far. Any pointer may be NULL. GM_ESTATE without a dense metric. */
int gm_hmc_get_dense_metric(gm_sampler* s, double* minv, double* a_factor, int64_t* updates, int64_t* failed);

/* MetropolisHastings::new (metropolis_hastings.rs:151-161) with an
 * IsotropicGaussian proposal of standard deviation proposal_std
 * (distributions.rs:349-390), driven like ChainRunner::run (core.rs:219-229). */
int gm_mh_create(const gm_target* target, gm_dtype dtype, int64_t n_chains, int64_t dim,
                 const void* init, double proposal_std, int64_t chain_offset,
                 gm_sampler** out);

/* ---- MH warm-up: a per-chain proposal scale and a per-chain diagonal shape ----
 * No reference counterpart (the reference's MH takes one IsotropicGaussian).
 * A sampler on which none of these calls was made runs exactly as before.
 * They need an MH sampler (GM_ESTATE otherwise).
 *
 * With per-chain state a transition of chain c proposes
 *   y[i] = x[i] + z[i] * f[i],   f[i] = scale[c] * diag[c][i]
 * from the plain path's proposal normals z (f rounded to the sampler dtype
 * once per chain, coordinate and scale value; product and sum are two
 * roundings) and accepts iff lp(y) - lp(x) > ln u: the proposal is symmetric.
 * diag is a standard deviation per coordinate, all ones unless set or adapted;
 * with diag == 1 and scale[c] == s the transition has the bits of the plain
 * path at proposal_std = s. The per-chain path exists where the plain kernel
 * drops the proposal's cancelling log-density terms: every scale finite and
 * > 0 with 2 scale^2 a normal number of the sampler dtype and a finite
 * proposal constant (GM_EINVAL otherwise, the sampler unchanged; the creation
 * proposal_std is held to the same when these calls start from it).
 *
 * gm_mh_set_adaptation arms a warm-up exactly as gm_hmc_set_adaptation does:
 * the n_discard transitions of the next gm_run* call adapt (n_discard == 0
 * adapts nothing and stays armed; gm_step never starts one; calling it again
 * re-arms from the current scales). Mode 1 adapts the scale per chain after
 * every warm-up transition by the dual averaging of the HMC warm-up (gamma
 * .05, t0 10, kappa .75, mu = ln(10 scale) at the start and at each restart)
 * on alpha = min(1, exp(log_alpha)), NaN -> 0; after the last warm-up
 * transition scale = scale_bar. Mode 2 adds Welford statistics of the
 * post-accept position while start_buffer < m < n_discard - end_buffer in the
 * windows of the shared schedule (initial_window doubling up to 400); at a
 * window end with >= 5 positions diag = sqrt(max((1 - regularize) var +
 * regularize, max(jitter, 1e-10))), the statistics reset and the dual
 * averaging restarts from scale_bar. Mode 0 drops all per-chain state: the
 * sampler is back on the creation proposal_std, the plain kernel and the
 * plain checkpoint. Recommended: target_accept 0.234, buffers 75 / 150,
 * initial_window 25, regularize 0.05, jitter 1e-6.
 * GM_EINVAL unless 0 < target_accept < 1, the window sizes are >= 0,
 * regularize is in [0, 1] and mode is 0, 1 or 2. */
int gm_mh_set_adaptation(gm_sampler* s, int32_t mode /* 0 off, 1 scale, 2 scale + diagonal shape */,
                         double target_accept, int64_t start_buffer, int64_t end_buffer,
                         int64_t initial_window, double regularize, double jitter);
/* Per-chain proposal scales scale[n_chains] (rounded to the sampler dtype);
 * scale_bar is set to the same values. */
int gm_mh_set_proposal_scales(gm_sampler* s, const double* scale);
/* Per-chain (scale, scale_bar), [n_chains] each, either may be NULL; the
 * creation proposal_std for every chain before any of these calls. */
int gm_mh_get_proposal_scales(gm_sampler* s, double* scale, double* scale_bar);
/* The proposal shape diag [n_chains][dim] of the sampler dtype, every entry
 * finite and > 0 (GM_EINVAL otherwise, the sampler unchanged). */
int gm_mh_set_proposal_diag(gm_sampler* s, const void* diag);
/* diag [n_chains][dim] of the sampler dtype; ones before any of these calls. */
int gm_mh_get_proposal_diag(gm_sampler* s, void* diag);

/* NUTS::new (nuts.rs:156-180) -> GenericNUTS::new (generic_nuts.rs:370-377):
 * identity mass matrix, dual-averaging step size (gamma .05, t0 10, kappa .75).
 * max_depth bounds the doubling loop (the reference has no bound,
 * generic_nuts.rs:782); pass 0 for the engine default (10). */
int gm_nuts_create(const gm_target* target, gm_dtype dtype, int64_t n_chains, int64_t dim,
                   const void* init, double target_accept_p, int32_t max_depth,
                   int64_t chain_offset, gm_sampler** out);

/* set_seed: hmc.rs:143-148, generic_nuts.rs:550-556, metropolis_hastings.rs:189-197.
 * Resets the sampler's transition counter so a re-seeded sampler replays. */
int gm_set_seed(gm_sampler* s, uint64_t seed);

/* One transition of every chain (HMC::step hmc.rs:316-318 /
 * BatchedGenericHMC::step batched_hmc.rs:129-163 / MHMarkovChain::step
 * metropolis_hastings.rs:306-318 / GenericNUTSChain::step generic_nuts.rs:755-925). */
int gm_step(gm_sampler* s);

/* run(n_collect, n_discard): hmc.rs:164-181, core.rs:219-229, nuts.rs:214-259.
 * out: host [n_chains][n_collect][dim] (may be NULL to skip the copy).
 * Step-count semantics follow the reference per sampler kind:
 *   HMC, MH: n_discard + n_collect transitions, every post-burn-in state kept;
 *   NUTS:    n_discard + n_collect - 1 transitions, row r = state after
 *            n_discard + r transitions (row 0 = start when n_discard == 0). */
int gm_run(gm_sampler* s, int64_t n_collect, int64_t n_discard, void* out);

/* run_positions (batched_hmc.rs:115-123): same transitions, samples stay on
 * the device as [n_collect][n_chains][dim]; *dev_samples is owned by the
 * sampler and valid until the next run/destroy. */
int gm_run_device(gm_sampler* s, int64_t n_collect, int64_t n_discard, const void** dev_samples);

/* NUTS::run_progress semantics (generic_nuts.rs:675-717): n_discard + n_collect
 * transitions, row r = state after n_discard + r + 1 transitions. Other
 * sampler kinds: identical to gm_run_device. */
int gm_run_device_progress(gm_sampler* s, int64_t n_collect, int64_t n_discard,
                           const void** dev_samples);

/* run_progress (hmc.rs:245-306, generic_nuts.rs:414-548, core.rs:251-403)
 * without the terminal UI: the transitions of gm_run_device_progress, samples
 * copied to host [n_chains][n_collect][dim] (out may be NULL), and the
 * device-side split R-hat / ESS of the collected draws (RunStats::from,
 * stats.rs:383-394) in rhat_out/ess_out [dim] (may be NULL; needs n_collect >= 2). */
int gm_run_progress(gm_sampler* s, int64_t n_collect, int64_t n_discard, void* out,
                    float* rhat_out, float* ess_out);

/* Copy the samples of the last run (device [n_collect][n_chains][dim]) to host
 * in the reference layout [n_chains][n_collect][dim]. n_rows must equal that
 * run's n_collect (the size of `out` in rows): GM_EINVAL otherwise, so a
 * buffer sized for an earlier, smaller run is never overrun. */
int gm_copy_samples(gm_sampler* s, int64_t n_rows, void* out);

/* A block of the last run's device samples, rows [row0, row0+n_rows) x
 * chains [chain0, chain0+n_chains), copied to the host as
 * [n_rows][n_chains][dim] (one strided copy): the streaming egress used by
 * the CSV / Arrow / Parquet writers (io/csv.rs, io/arrow.rs, io/parquet.rs) so that a sample larger than
 * host memory never has to exist there whole. */
int gm_copy_sample_block(gm_sampler* s, int64_t row0, int64_t n_rows, int64_t chain0, int64_t n_chains,
                         void* out);
/* positions() (hmc.rs:326-328): host [n_chains][dim]. */
int gm_get_positions(gm_sampler* s, void* out);
int gm_set_positions(gm_sampler* s, const void* in);

/* Per-chain count of accepted transitions since creation / set_seed
 * (the quantity behind MultiChainTracker::p_accept, stats.rs:238-269). */
int gm_get_accept_counts(gm_sampler* s, int64_t* out);

/* HMC and MH: the log-density of each chain's current position as the last
 * launch computed it ([n_chains] of the sampler's dtype). GM_ESTATE before the
 * first transition and for NUTS. Tests and diagnostics. */
int gm_get_logp(gm_sampler* s, void* out);

/* Per-chain count of leapfrog steps integrated since creation (HMC:
 * n_leapfrog per transition; NUTS: the tree sizes actually built; MH: 0). */
int gm_get_leapfrog_counts(gm_sampler* s, int64_t* out);

/* ---- Per-transition sampler statistics (HMC, NUTS) --------------------------
 * No reference counterpart. mode 0 off (the default), 1 "collected": a record
 * for every transition whose resulting state is a collected sample row,
 * 2 "all": for every transition of a run, warm-up first. A run option, not
 * sampler state: checkpoints (gm_state_save) do not contain it, and samples,
 * counts, step sizes and metrics are bit for bit those of a run without it.
 * gm_run, gm_run_device, gm_run_device_progress, gm_run_progress and
 * gm_run_progress_cb record; gm_step does not. The records of a run are
 * [n_transitions][n_chains] on the device, owned by the sampler and valid
 * until its next run or destroy. GM_ESTATE for MH, GM_EINVAL for HMC on a wide
 * layout (dim > 1024). A plain HMC sampler records through the kernel of the
 * per-chain step sizes with the identity metric (the same bits).
 *
 * One record, of the sampler's dtype T (16 bytes f32, 32 bytes f64, aligned
 * to its size):
 *   T energy       K(p0) - logp(q) after the momentum refresh
 *   T accept_stat  NUTS: alpha / n_alpha; HMC: min(1, exp(log_alpha)), NaN -> 0
 *   T step_size    the step size the transition integrated with
 *   word           uint32 (f32) / uint64 (f64, upper half 0):
 *                  bits 0-23 n_leapfrog (saturates at 2^24 - 1), 24-29
 *                  tree_depth (HMC 0), 30 divergent (NUTS: a leaf failed
 *                  (logu - 1000) < joint; HMC: !(log_alpha > -1000)),
 *                  31 accepted (the transition moved the chain) */
int gm_sampler_set_stats(gm_sampler* s, int32_t mode);

/* The last run's records: how many transitions were recorded, the index
 * (within the records) of the first one whose resulting state is a collected
 * sample row, the sample row that state is (0; 1 after a NUTS gm_run with
 * n_discard 0, whose row 0 is the start state and has no transition) and the
 * bytes of one record. Record first_collected + k belongs to sample row
 * first_row + k. Any output may be NULL. GM_ESTATE when the last run recorded
 * nothing (this and the getters below synchronise an asynchronous run first). */
int gm_sampler_stats_info(gm_sampler* s, int64_t* n_transitions, int64_t* first_collected, int64_t* first_row,
                          int32_t* record_bytes);
/* The records on the device, [n_transitions][n_chains]. */
int gm_sampler_stats_device(gm_sampler* s, const void** records);

typedef enum {
  GM_STAT_ENERGY = 0,      /* T */
  GM_STAT_ACCEPT_STAT = 1, /* T */
  GM_STAT_STEP_SIZE = 2,   /* T */
  GM_STAT_N_LEAPFROG = 3,  /* int32 */
  GM_STAT_TREE_DEPTH = 4,  /* int32 */
  GM_STAT_DIVERGENT = 5,   /* uint8 */
  GM_STAT_ACCEPTED = 6     /* uint8 */
} gm_stat_field;
/* One field of the last run's records on the host, [n_chains][n_transitions]. */
int gm_sampler_stats_field(gm_sampler* s, int32_t field, void* out);

/* The device reduction of record rows [row0, row0 + n_rows), in float64:
 * per_chain [GM_STATS_FIELDS][n_chains] and the chains' totals
 * total [GM_STATS_FIELDS] (either may be NULL). E-BFMI is
 * sum (E_n - E_{n-1})^2 / sum (E_n - mean E)^2; its total pools the chains'
 * sums, each about its own mean. Rows whose energy is not finite are counted
 * (N_SKIPPED) and left out of both energy sums; a difference needs both of
 * its adjacent rows finite. The other quantities take every row. */
enum {
  GM_STATS_EBFMI = 0,
  GM_STATS_N_DIVERGENT = 1,
  GM_STATS_MEAN_ACCEPT = 2,
  GM_STATS_MEAN_LEAPFROG = 3,
  GM_STATS_MEAN_DEPTH = 4,
  GM_STATS_N_MAX_DEPTH = 5, /* transitions whose tree reached max_depth (HMC: 0) */
  GM_STATS_N_ENERGY = 6,    /* rows with a finite energy */
  GM_STATS_N_SKIPPED = 7,   /* rows without */
  GM_STATS_FIELDS = 8
};
int gm_sampler_stats_reduce(gm_sampler* s, int64_t row0, int64_t n_rows, double* per_chain, double* total);
/* The same reduction of records the caller holds on the device
 * ([.][n_chains] of dtype's record). max_depth 0: nothing counts as having
 * reached it. */
int gm_stats_reduce_device(const void* records, gm_dtype dtype, int64_t n_chains, int64_t row0, int64_t n_rows,
                           int32_t max_depth, double* per_chain, double* total);

/* NUTS per-chain adaptation state: step size epsilon and epsilon_bar
 * (generic_nuts.rs:573-582). Pass NULL to skip either. */
int gm_nuts_get_step_size(gm_sampler* s, double* eps, double* eps_bar);

/* Mass-matrix warm-up, GenericNUTS::new_with_mass_matrix (generic_nuts.rs:
 * 33-65, 379-398): mode 0 none (NUTS::new), 1 diagonal, 2 dense (falls back
 * to diagonal when dim > dense_max_dim). During warm-up (m <= n_discard) the
 * positions inside the window (start_buffer < m < n_discard - end_buffer)
 * feed a Welford covariance; at each window end (initial_window, doubling
 * up to 400) the metric becomes (1-regularize)*cov + regularize (diagonal
 * floored at jitter), the step size is re-found from a probe momentum and
 * dual averaging restarts (:897-921, 948-997). Resets the metric to identity
 * and the window schedule to its start; call before the first run. A dense
 * metric runs on a one-wave layout: once the mode is accepted, a wide layout
 * (lanes > 64) is replaced by the default one, and restored when a later call
 * selects mode 0 or 1; on an error the layout is unchanged. */
int gm_nuts_set_mass_adaptation(gm_sampler* s, int32_t mode, int64_t start_buffer, int64_t end_buffer,
                                int64_t initial_window, double regularize, double jitter,
                                int64_t dense_max_dim);
/* The convention of the metric that the warm-up's window ends write, from
 * the next window end on (no reference counterpart beyond the default).
 * convention 0 (the default) is the reference's, M = Sigma_hat: the slots
 * that gm_nuts_get_mass reads hold Sigma_hat^-1 (or 1/var) and
 * chol(Sigma_hat) (or sqrt(var)). convention 1 is the whitening one,
 * M^-1 = Sigma_hat (Stan's): the same slots hold Sigma_hat (or var) and
 * chol(Sigma_hat^-1) (or 1/sqrt(var)), from the same statistics, floors and
 * jitter tries; the sampling kernels are the same and take either as the
 * same pair of operators. pooled 1 (whitening only, 2 <= dim <= 64, else
 * GM_EINVAL) estimates one Sigma_hat in float64 from the window rows of all
 * chains of the sampler instead of one per chain, n = rows * n_chains:
 * Sigma_hat = (1 - regularize) S + regularize I, diagonal floored at
 * max(jitter, 1e-10); a window of fewer than 5 rows changes nothing; a
 * non-positive or non-finite pivot keeps the previous metric and is counted.
 * Every chain's slots get the same matrices, rounded once to the sampler
 * dtype. The setting survives gm_nuts_set_mass_adaptation. A failed call
 * leaves the sampler as it was. */
int gm_nuts_set_metric_convention(gm_sampler* s, int32_t convention, int32_t pooled);
/* The pooled metric's float64 masters, Sigma_hat and the lower Cholesky
 * factor of its inverse ([dim][dim] each), and the numbers of window ends
 * that replaced the metric / kept it after a failed factorisation. Any output
 * may be NULL. GM_ESTATE unless the whitening convention is set at
 * 2 <= dim <= 64. */
int gm_nuts_get_pooled_metric(gm_sampler* s, double* sigma, double* chol_prec, int64_t* updates,
                              int64_t* failed);
/* sigma (float64 [dim][dim]: finite, exactly symmetric, positive definite,
 * else GM_EINVAL) as every chain's dense whitening metric, factored on the
 * device as at a window end; e.g. a metric warmed up by a sampler with fewer
 * chains. Needs mode 2 and the whitening convention (GM_ESTATE otherwise).
 * Step sizes, counters and warm-up state are untouched. A failed call leaves
 * the sampler as it was. */
int gm_nuts_set_pooled_metric(gm_sampler* s, const double* sigma);
/* The current metric: mode, per-chain kind [C] (0 identity, 1 diagonal,
 * 2 dense), diagonal inverse and sqrt [C][dim], dense inverse and Cholesky
 * factor [C][dim][dim] (mode 2). Any output may be NULL. */
/* Where a NUTS sampler keeps the levels of its subtree stack (the stored
 * left siblings of build_tree's recursion): the first `levels` in LDS, deeper
 * ones in HBM; -1 (the default) puts as many in LDS as fit next to the
 * target's staging area. Results are identical for every value. */
int gm_nuts_set_lds_levels(gm_sampler* s, int32_t levels);

/* Where a dense-metric NUTS sampler (layout 16 x 2, dim <= 32) keeps each
 * chain's M^-1 and Cholesky factor: minv_lds 1 (the default, also -1) the
 * packed lower triangles in LDS, which leaves room for 6 subtree-stack
 * levels on chip; 2 the full matrices when they fit next to the target's
 * staging (else packed: one stack level, ~10x the HBM traffic, ~2 % faster);
 * 0 global memory. chol_lds 1 also packs the Cholesky factor into LDS when
 * the packed M^-1 leaves room (default, also -1: 0). Every form gives
 * identical results (no reference counterpart: a placement choice of this
 * engine). */
int gm_nuts_set_dense_forms(gm_sampler* s, int32_t minv_lds, int32_t chol_lds);

/* The last NUTS launch's on-chip plan: plan[0] subtree-stack levels in LDS,
 * plan[1] M^-1 form (0 global, 1 packed, 2 full), plan[2] its LDS offset,
 * plan[3] Cholesky factor in LDS (0/1), plan[4] its offset, plan[5] 1 when
 * the launch ran the frozen-dense kernel (every chain's metric dense, no
 * warm-up window, the momentum pass on: GM_FROZEN_WAVES waves per SIMD).
 * The first min(cap, 6)
 * values are written to plan (cap >= 1); returns GM_OK. */
int gm_nuts_get_plan(gm_sampler* s, int32_t* plan, int32_t cap);

/* Where the NUTS transition momenta are drawn: on (default) in one parallel
 * pass per launch ahead of the tree kernel, into a [steps][C][D] buffer that
 * the sampler keeps for its later launches (at most 4 GiB and a quarter of
 * the device memory free when it grows; a launch it does not fit draws in the
 * kernel), off in the tree kernel at each transition start (switching it off
 * releases the buffer). With a dense metric the pass also applies it (the
 * momenta L z and their M^-1 L z, in a second [steps][C][D] buffer) for the
 * frozen-dense kernel, which needs it: with the pass off those launches run
 * the adaptive dense kernel. The same Philox/Box-Muller values and the same
 * sums either way (identical results); no reference counterpart. */
int gm_nuts_set_momentum_pass(gm_sampler* s, int32_t on);

int gm_nuts_get_mass(gm_sampler* s, int32_t* mode, int32_t* kind, void* dinv, void* dsqrt, void* minv,
                     void* mchol);

/* Lane layout the kernels use for this sampler: `lanes` lanes cooperate on
 * one chain, each holding `elems` consecutive coordinates. Per-chain sums
 * (kinetic energy, log-density) are reduced lane-sequentially then by an xor
 * butterfly over the lanes, which fixes the floating-point summation order. */
int gm_sampler_layout(gm_sampler* s, int32_t* lanes, int32_t* elems);
int gm_sampler_set_layout(gm_sampler* s, int32_t lanes, int32_t elems);

/* Device time (ms) of the sampling kernels launched by the last run, and the
 * number of launches (HIP events on the sampler's stream). */
int gm_sampler_last_run_stats(gm_sampler* s, double* kernel_ms, int64_t* launches);

/* Asynchronous runs (HMC and MH samplers; NUTS runs stay synchronous):
 * with on != 0, gm_run_device / gm_step return once the sampler's kernels
 * are enqueued on its stream instead of waiting for them. The caller then
 * waits with gm_sampler_synchronize or gm_device_synchronize before reading
 * the samples from another stream (the diagnostics, gm_memcpy_*); the
 * sampler's own calls (copies, positions, state) are ordered after the run
 * on its stream. A benchmark that brackets a run with device synchronizes
 * uses it to wait once instead of twice. */
int gm_sampler_set_async(gm_sampler* s, int32_t on);
int gm_sampler_synchronize(gm_sampler* s);

/* Transitions per kernel launch (state stays in registers inside a launch). */
int gm_sampler_set_steps_per_launch(gm_sampler* s, int64_t steps);

/* HMC leapfrog-loop form of the fused kernel: 0 (default) chosen by the
 * launch's waves per SIMD and L, or forced to 1, 2 or 4 leapfrogs per loop
 * trip, to 7, the long count-down form (7 per trip after (L - 1) % 7 single
 * ones; the kernels that do not compile it in run it as 1), or to 49, the
 * block form ((L - 1) % 49 leapfrogs as straight-line pieces of 1, 2, 4, ...,
 * then count-down passes of 49 straight-line ones; the kernels that do not
 * compile it in run it as 7, or as 1). Tests and measurements; identical
 * results in every form. No reference counterpart. */
int gm_sampler_set_unroll(gm_sampler* s, int32_t n);
/* The form the last run's HMC launches took (the automatic choice resolved). */
int gm_sampler_last_unroll(gm_sampler* s, int32_t* n);

/* HMC draw-wave form of the fused kernel: the momenta, their kinetic energies
 * and the accept log-uniforms of a draw block are made by waves of their own
 * beside the chain waves of a workgroup and handed over through LDS, one
 * barrier per draw block. -1 (default) chosen by the regime in which it
 * measured faster, 0 off, or n = 1, 2 or 4 draw waves per 4 chain waves
 * forced. The form is compiled for the block leapfrog form (unroll 49: one
 * chain per wave, one element per lane, RosenbrockND; a forced n takes that
 * loop form with it where the unroll is automatic) at n = 1; a launch that
 * is not of that kind, or another n, runs as off. Refused (n > 0) while
 * sampler statistics are on. Tests and measurements; identical results
 * either way. No reference counterpart. */
int gm_sampler_set_draw_waves(gm_sampler* s, int32_t n);
/* The draw waves per workgroup of the last run's HMC launches (0: the form
 * was off). */
int gm_sampler_last_draw_waves(gm_sampler* s, int32_t* n);

/* Pre-size the device sample buffer for runs collecting up to n_collect
 * transitions, so that a later gm_run / gm_run_device does no device
 * allocation (the buffer only grows; hmc.rs:164-181 allocates its output on
 * every run). */
int gm_sampler_reserve(gm_sampler* s, int64_t n_collect);

/* Checkpoint / resume. The reference keeps a sampler's state only in the
 * object between run calls (batched_hmc.rs:40; generic_nuts.rs:573-582, 744)
 * and leaves checkpointing as a TODO (core.rs:177). gm_state_save writes that
 * state (positions, accept / leapfrog counts, seed and stream position; NUTS
 * step-size adaptation, metric and warm-up schedule) to a caller-owned host
 * buffer of gm_state_size bytes; gm_state_load restores it into a sampler
 * created with the same kind, dtype, n_chains, dim and chain_offset, which
 * then continues the same random streams bit for bit. */
int gm_state_size(gm_sampler* s, uint64_t* bytes);
int gm_state_save(gm_sampler* s, void* out, uint64_t bytes);
int gm_state_load(gm_sampler* s, const void* in, uint64_t bytes);

int gm_destroy(gm_sampler* s);

/* ---- diagnostics (stats.rs) ---------------------------------------------
 * split_rhat_mean_ess (stats.rs:439-450, Appendix B of SURVEY.md): returns
 * split R-hat = sqrt(W/V) (the reference's orientation, stats.rs:452-454) and
 * ESS per parameter, as f32, like the reference.
 * Host variant: sample is host [n_chains][n_draws][n_params] (reference
 * layout). Device variant: sample is a device pointer with explicit element
 * strides (chain, draw, param). */
int gm_split_rhat_ess(const void* sample, gm_dtype dtype, int64_t n_chains, int64_t n_draws,
                      int64_t n_params, float* rhat_out, float* ess_out);
int gm_split_rhat_ess_device(const void* dev_sample, gm_dtype dtype, int64_t n_chains,
                             int64_t n_draws, int64_t n_params, int64_t stride_chain,
                             int64_t stride_draw, int64_t stride_param, float* rhat_out,
                             float* ess_out);

/* ---- posterior summary (not in the reference) ----------------------------
 * Location, scale, quantiles and the rank-normalised diagnostics of Vehtari
 * et al. 2021 per parameter, computed on the device from a [C][N][P] sample
 * (N >= 4). With h = N / 2, Y the 2C split chains (first and last h draws of
 * each chain; an odd N's middle draw is in none) and M = 2 C h pooled values:
 *   ranks      1-based average ranks of Y among the M pooled values, in the
 *              sample's own dtype (-0 == +0; an f64 sample is never rounded)
 *   z          Phi^-1((r - 3/8) / (M + 1/4))
 *   ess_bulk   ESS of the Appendix-B estimator (the one behind
 *              gm_split_rhat_ess) applied to z
 *   rhat       max over z and z_fold of sqrt(V/W): the usual orientation,
 *              >= 1 when chains disagree (gm_split_rhat_* report sqrt(W/V) and
 *              keep doing so). z_fold are the normal scores of |Y - median|,
 *              formed and ranked in f64
 *   ess_tail   min of the ESS of I(Y <= y_(k05)) and of I(Y <= y_(k95)), y_(k)
 *              the 0-based k-th pooled order statistic, k_q = floor((M-1) q)
 *   quantiles  of Y, linear interpolation between order statistics
 *              (numpy.quantile's default), in f64
 *   mean, sd   over all C N draws, sd with ddof = 1, in f64
 * Unlike Stan the ESS has no M log10(M) cap. A parameter whose pooled values
 * hold a NaN or an infinity reports NaN in every field; one whose pooled
 * values are all equal reports NaN for rhat, ess_bulk and ess_tail and its
 * exact mean and quantiles.
 * Every entry point returns GM_EINVAL before any device call for a bad dtype,
 * a NULL sample or out, n_chains < 1, n_draws < 4, n_params < 1, n_probs
 * outside [0, 32], a prob outside [0, 1] (or NaN), or M >= 2^31.
 * Host variant: sample is host [n_chains][n_draws][n_params]. Device variant:
 * a device pointer with element strides (chain, draw, param). */
typedef struct gm_summary_out { /* host arrays, any may be NULL */
  double* mean;      /* [P] */
  double* sd;        /* [P] */
  double* quantiles; /* [n_probs][P] */
  double* rhat;      /* [P] rank-normalised, max(bulk, folded), sqrt(V/W) */
  double* ess_bulk;  /* [P] */
  double* ess_tail;  /* [P] */
} gm_summary_out;
int gm_summary(const void* sample, gm_dtype dtype, int64_t n_chains, int64_t n_draws,
               int64_t n_params, int32_t n_probs, const double* probs, gm_summary_out* out);
int gm_summary_device(const void* dev_sample, gm_dtype dtype, int64_t n_chains, int64_t n_draws,
                      int64_t n_params, int64_t stride_chain, int64_t stride_draw,
                      int64_t stride_param, int32_t n_probs, const double* probs,
                      gm_summary_out* out);
/* Ranks (exact, multiples of 1/2) and normal scores of the pooled split draws
 * of a host sample, as host [C][N][P] f64 with NaN in an odd N's middle draw;
 * folded != 0: those of |x - median|. Either output may be NULL. */
int gm_rank_normalize(const void* sample, gm_dtype dtype, int64_t n_chains, int64_t n_draws,
                      int64_t n_params, int32_t folded, double* ranks_out, double* z_out);
/* The sort's internal sizes, for tests: [0] the largest M of the
 * one-workgroup (LDS) path, [1] elements per block of the global radix path,
 * [2] radix bits per pass, [3] parameters per chunk at most. Writes
 * min(cap, 4) values. */
int gm_summary_sort_plan(int32_t* out, int32_t cap);

/* ---- GLM posterior prediction over stored draws -------------------------
 * Not in the reference. For a GLM (gm_glm_desc: family, x [n_rows][dim], an
 * optional offset, an optional y; prior_sd is ignored and may be NULL) and
 * n_draws coefficient vectors theta_s of dtype T, per draw s and row m in T:
 *   eta = offset_m + sum_j x[m][j] theta_sj    (from offset_m, columns
 *                                               ascending, one fma each)
 *   mu  = logistic(eta) | exp(eta)             (no overflow for Bernoulli)
 *   ll  = (y_m eta - A(eta)) + c_m             c_m = -lgamma(y_m + 1) for
 *                                              poisson_log, 0 for
 *                                              bernoulli_logit, computed in
 *                                              float64 and rounded to T
 * and per row m, reduced over all draws in float64:
 *   eta_mean, eta_sd, mu_mean, mu_sd   sample mean and sd (ddof = 1)
 *   lppd                               log((1/S) sum_s exp ll), running maximum
 *   ll_mean, ll_var                    sample mean and variance (ddof = 1)
 * With n_draws = 1 the sd and variance outputs are NaN. A row whose ll is
 * -inf in every draw has lppd = -inf; -inf in some draws adds 0 to the lppd
 * sum and makes ll_mean -inf and ll_var NaN; a NaN in a draw makes that
 * row's outputs NaN. WAIC: elpd_m = lppd_m - ll_var_m.
 * pointwise: the matrix ll [n_draws][n_rows] of dtype, copied to the host;
 * refused when it would be larger than 2^31 bytes (pass the rows in blocks).
 * lppd, ll_mean, ll_var and pointwise need y. eta is formed on the matrix
 * cores; the split of the work depends on (n_draws, n_rows, dim, dtype) only,
 * so repeated calls, the host and the device entry point, and two devices
 * give the same bits.
 * Every entry point returns GM_EINVAL before any device call, with
 * gm_target's wording and first-offender rule for the model ("GLM target:
 * ..."), for: a NULL model, x, draws or out; a bad family, dim outside
 * [1, 128], n_rows outside [1, 2^24]; a bad dtype; n_draws < 1; stride_draw <
 * dim; an output that needs y without y; a pointwise matrix over the cap; a
 * non-finite x, y or offset; y outside the family's range.
 * Host variant: draws is host [n_draws][dim]. Device variant: a device
 * pointer to n_draws rows, stride_draw elements apart. */
typedef struct gm_glm_predict_out { /* host arrays [n_rows], any may be NULL */
  double *eta_mean, *eta_sd, *mu_mean, *mu_sd, *lppd, *ll_mean, *ll_var;
  void* pointwise; /* host [n_draws][n_rows] of dtype, or NULL */
} gm_glm_predict_out;
int gm_glm_predict(const gm_glm_desc* model, int64_t dim, gm_dtype dtype,
                   const void* draws /* host [n_draws][dim] */, int64_t n_draws,
                   gm_glm_predict_out* out);
int gm_glm_predict_device(const gm_glm_desc* model, int64_t dim, gm_dtype dtype,
                          const void* dev_draws, int64_t n_draws, int64_t stride_draw,
                          gm_glm_predict_out* out);
/* The decomposition's sizes, for tests: [0] draws per slab, [1] data rows per
 * workgroup tile, [2] draws per matrix-core tile. Writes min(cap, 3) values. */
int gm_glm_predict_plan(int32_t* out, int32_t cap);

/* ---- GLM PSIS-LOO over stored draws -------------------------------------
 * Not in the reference. Pareto-smoothed importance-sampling leave-one-out
 * (Vehtari, Simpson, Gelman, Yao & Gabry 2024) per data row m of a GLM with y,
 * from the pointwise log-likelihood ll_s (s = 1 .. S = n_draws) of
 * gm_glm_predict: same operations, same dtype T, same bits. In float64:
 *   lw_s = -ll_s - max_s(-ll_s)
 *   M    = min(floor(0.2 S), ceil(3 sqrt(S / reff)))        (tail_len)
 *   M < 5: pareto_k = +inf, nothing is smoothed. Otherwise the tail is the M
 *   largest lw, cutoff = max(largest lw outside the tail, log(DBL_MIN)),
 *   x_j = exp(tail_j) - exp(cutoff), j = 1 .. M ascending. x_M <= 0 or
 *   x_(floor(M/4 + 0.5)) <= 0: pareto_k = +inf, nothing is smoothed. Otherwise
 *   the generalised Pareto fit of Zhang & Stephens (2009): m = 30 +
 *   floor(sqrt M) grid points theta_j = 1/x_M + (1 - sqrt(m / (j - 0.5))) /
 *   (3 x_(floor(M/4 + 0.5))), kappa(theta) = mean_i log1p(-theta x_i),
 *   l_j = M (log(-theta_j / kappa_j) - kappa_j - 1), w_j = 1 / sum_j' exp(l_j'
 *   - l_j), theta^ = sum_j theta_j w_j, k = kappa(theta^), sigma = -k / theta^,
 *   then k <- (k M + 5) / (M + 10). A finite k replaces tail value j by
 *   min(log(sigma expm1(-k log1p(-p_j)) / k + exp(cutoff)), 0), p_j =
 *   (j - 0.5) / M (k = 0: -sigma log1p(-p_j)); a non-finite k leaves the tail
 *   and is reported as it came out.
 *   elpd_loo = logsumexp_s(lw_s + ll_s) - logsumexp_s(lw_s), smoothed lw.
 * n_draws = 1 gives elpd_loo = ll_1 and pareto_k = +inf. A row with a
 * non-finite ll (NaN, +inf or -inf) in any draw has elpd_loo = pareto_k = NaN
 * (its tail too) and is counted in n_nonfinite.
 * tail: the raw (unsmoothed) tail of every row, float64 [n_rows][tail_len]
 * ascending; the caller sizes it with gm_glm_loo_plan. The lppd that p_loo
 * needs is gm_glm_predict's.
 * Workspace: rows are taken in groups of R, a multiple of 64; a group holds
 * ll [R][n_draws rounded up to 4] of T, 2 P float64 slots a row (P the power
 * of two >= tail_len + 1) and 20 bytes a row. R is the largest multiple of 64
 * that workspace_bytes holds (0: the default, 2^32 + 2^28), at most n_rows rounded
 * up to 64 and 2^20. n_draws <= 2^24; tail_len has no limit of its own. The
 * workspace must hold 64 rows: at the default that is every n_draws up to
 * 2^24 in f32 and up to about 8.8e6 in f64 (reff = 1); beyond it the caller
 * passes a larger workspace_bytes (gm_glm_loo_plan [5] is the largest n_draws
 * that fits). The bound covers the per-group buffers above only, not the model
 * (x padded to 4 k-steps, offset, y, c of T) nor, in gm_glm_loo, the uploaded
 * copy of the draws. elpd_loo is formed with one logarithm of the quotient of
 * the two sums, not as the difference of two log-sums of the size of log S. No
 * floating-point atomics; every sum has a fixed order that depends on
 * (n_draws, tail_len) only, so repeated calls, the host and the device entry
 * point, and any workspace_bytes give the same bits.
 * GM_EINVAL before any device call, with gm_glm_predict's wording for the
 * model ("GLM target: ..."), for everything gm_glm_predict refuses, and for:
 * a NULL y; reff not finite or <= 0; n_draws > 2^24; workspace_bytes < 0 or
 * too small for 64 rows (the message gives the bytes needed). */
typedef struct gm_glm_loo_out {
  double *elpd_loo, *pareto_k; /* host [n_rows], either may be NULL */
  double* tail;                /* host [n_rows][tail_len], or NULL */
  int64_t tail_len;            /* written: M */
  int64_t n_nonfinite;         /* written: rows with a non-finite ll */
} gm_glm_loo_out;
int gm_glm_loo(const gm_glm_desc* model, int64_t dim, gm_dtype dtype,
               const void* draws /* host [n_draws][dim] */, int64_t n_draws, double reff,
               int64_t workspace_bytes, gm_glm_loo_out* out);
int gm_glm_loo_device(const gm_glm_desc* model, int64_t dim, gm_dtype dtype,
                      const void* dev_draws, int64_t n_draws, int64_t stride_draw, double reff,
                      int64_t workspace_bytes, gm_glm_loo_out* out);
/* The split of such a call, without a device: [0] tail_len, [1] rows per
 * group, [2] workspace bytes used, [3] bytes per row, [4] the default
 * workspace_bytes, [5] the largest n_draws (<= 2^24) of which this dtype, reff
 * and workspace_bytes hold 64 rows, [6] sort slots per row. Writes
 * min(cap, 7) values; refuses what the call would refuse of these arguments. */
int gm_glm_loo_plan(gm_dtype dtype, int64_t n_draws, int64_t n_rows, double reff,
                    int64_t workspace_bytes, int64_t* out, int32_t cap);

/* ---- multi-GPU (one process per GPU, RCCL over xGMI) -------------------
 * Chains are sharded in contiguous blocks; sampling needs no communication.
 * The only exchange is an RCCL all-gather of per-split-chain summaries for
 * split-R-hat/ESS. */
typedef struct gm_comm gm_comm;
#define GM_UNIQUE_ID_BYTES 128
int gm_comm_get_unique_id(void* id_out /* GM_UNIQUE_ID_BYTES */);
int gm_comm_init(const void* id, int32_t nranks, int32_t rank, gm_comm** out);
int gm_comm_destroy(gm_comm* comm);
/* What RCCL itself reports for the communicator (ncclCommCount,
 * ncclCommUserRank, ncclCommCuDevice): the ranks the exchange really spans.
 * Any pointer may be NULL. */
int gm_comm_info(gm_comm* comm, int32_t* nranks, int32_t* rank, int32_t* device);
/* Same result on every rank: diagnostics of the union of all ranks' chains
 * (rank r holds global chains [offset_r, offset_r + n_chains_local)).
 * Every rank must pass the same (n_chains_local, n_draws, n_params, dtype).
 * The first call with a given shape on a communicator checks that with one
 * small all-gather (a mismatch is GM_EINVAL on every rank); later calls with
 * that shape go straight to the one grouped all-gather of the summaries. */
int gm_split_rhat_ess_dist(gm_comm* comm, const void* dev_sample, gm_dtype dtype,
                           int64_t n_chains_local, int64_t n_draws, int64_t n_params,
                           int64_t stride_chain, int64_t stride_draw, int64_t stride_param,
                           float* rhat_out, float* ess_out);
/* The same exchange with all R shards on the calling thread's device
 * (equal chain counts, same strides): shard r's summaries land where the
 * all-gather puts rank r's, and one final kernel reads them. Equals
 * split_rhat_mean_ess (stats.rs:439-450) of the concatenated chains, up to
 * summation order; one process driving several shards uses it, and it
 * checks the multi-rank assembly on a single GPU. */
int gm_split_rhat_ess_shards(const void* const* dev_shards, int32_t n_shards, gm_dtype dtype,
                             int64_t n_chains_per_shard, int64_t n_draws, int64_t n_params,
                             int64_t stride_chain, int64_t stride_draw, int64_t stride_param,
                             float* rhat_out, float* ess_out);

/* ---- run_progress with live statistics -------------------------------
 * The reference's run_progress draws progress bars fed by chain trackers:
 * HMC steps a MultiChainTracker with the current positions at most every
 * 500 ms and at the last step (hmc.rs:245-306); ChainRunner (MH) and NUTS
 * step a ChainTracker per chain after EVERY transition, burn-in included,
 * and report collect_rhat over the chains every second (core.rs:132-176,
 * 251-387; generic_nuts.rs:675-716). Here the trackers live on the device
 * (MH / NUTS: fused into the sampling kernels) and `cb`, when not NULL, is
 * called between launches at most every `interval_s` seconds and after the
 * last transition. The returned samples and R-hat/ESS are those of
 * gm_run_progress. */
typedef struct gm_progress {
  int64_t done;   /* transitions done (HMC: of the n_collect phase; MH/NUTS: of all) */
  int64_t total;  /* HMC: n_collect; MH/NUTS: n_discard + n_collect */
  float p_accept; /* HMC: MultiChainTracker::p_accept; MH/NUTS: mean over chains of
                     the ChainTracker acceptance EMA */
  float max_rhat; /* max over parameters of the tracker R-hat, NaN skipped
                     (stats.rs:139-161, 298-317) */
} gm_progress;
typedef void (*gm_progress_fn)(void* user, const gm_progress* info);
int gm_run_progress_cb(gm_sampler* s, int64_t n_collect, int64_t n_discard, void* out,
                       float* rhat_out, float* ess_out, gm_progress_fn cb, void* user,
                       double interval_s);
/* ChainTracker::stats of every chain after an MH / NUTS run_progress
 * (stats.rs:122-131): steps taken, p_accept [C], mean [C][dim], sm2 [C][dim]
 * (any output may be NULL). */
int gm_sampler_chain_stats(gm_sampler* s, uint64_t* n, float* p_accept, float* mean, float* sm2);

/* MultiChainTracker (stats.rs:199-339) over [n_chains][n_params] device
 * positions of either dtype. */
typedef struct gm_mct gm_mct;
int gm_mct_create(int64_t n_chains, int64_t n_params, gm_mct** out);
int gm_mct_step(gm_mct* t, const void* dev_positions, gm_dtype dtype);
/* p_accept, rhat [n_params] and max_rhat (any may be NULL) */
int gm_mct_stats(gm_mct* t, float* p_accept, float* rhat, float* max_rhat);
int gm_mct_destroy(gm_mct* t);

/* ---- granular BatchVector ops (tier 2 of the boundary) ----------------
 * The reference's plug-in seam is the BatchVector trait implemented for
 * Tensor<B,2> [n_chains, dim] (euclidean.rs:145-195, 358-534) plus
 * BatchedHamiltonianTarget::logp_and_grad (batched_hmc.rs:18-22). These
 * entry points are those operations on caller-held DEVICE buffers, so a
 * BatchVector implementation (or BatchedGenericHMC::step itself,
 * batched_hmc.rs:129-190) can be driven op by op. A step composed of them
 * equals the fused gm_step bit for bit: same Philox streams (momentum:
 * tag 2, accept: tag 3, keyed by global chain id and step), same rounding,
 * and per-chain sums in the canonical order of the default layout of `dim`.
 * Matrices are [n_chains][dim] row-major, energies [n_chains], masks
 * uint8 [n_chains]. Ops are enqueued in order on the device's null stream;
 * gm_device_synchronize waits for them. */
int gm_malloc(void** dev_ptr, size_t bytes);
int gm_free(void* dev_ptr);
int gm_memcpy_htod(void* dev_dst, const void* host_src, size_t bytes);
int gm_memcpy_dtoh(void* host_dst, const void* dev_src, size_t bytes);
/* assign (euclidean.rs:380-382): dev_dst = dev_src */
int gm_memcpy_dtod(void* dev_dst, const void* dev_src, size_t bytes);

/* kinetic_energy (euclidean.rs:464-472): ke[c] = (sum_j p[c,j]^2) * 0.5 */
int gm_bv_kinetic_energy(gm_dtype dtype, int64_t n_chains, int64_t dim, const void* p, void* ke);
/* masked_assign (euclidean.rs:474-482): x[c,:] = other[c,:] where mask[c] != 0 */
int gm_bv_masked_assign(gm_dtype dtype, int64_t n_chains, int64_t dim, void* x, const void* other,
                        const uint8_t* mask);
/* add_scaled_assign (euclidean.rs:392-394): x = x + other * alpha, two
 * roundings, alpha rounded to dtype first; n = number of elements */
int gm_bv_add_scaled_assign(gm_dtype dtype, int64_t n, void* x, const void* other, double alpha);
/* fill_random_normal (euclidean.rs:484-496): out[c,j] = momentum draw of
 * chain chain_offset+c, coordinate j, transition `step` under `seed` */
int gm_bv_fill_random_normal(gm_dtype dtype, int64_t n_chains, int64_t dim, void* out, uint64_t seed,
                             uint32_t chain_offset, uint64_t step);
/* sample_uniform (euclidean.rs:498-509): out[c] in [0,1), the accept draw */
int gm_bv_sample_uniform(gm_dtype dtype, int64_t n_chains, void* out, uint64_t seed,
                         uint32_t chain_offset, uint64_t step);
/* energy_sub / energy_add / energy_neg / energy_ln (euclidean.rs:511-525) */
int gm_bv_energy_sub(gm_dtype dtype, int64_t n, const void* a, const void* b, void* out);
int gm_bv_energy_add(gm_dtype dtype, int64_t n, const void* a, const void* b, void* out);
int gm_bv_energy_neg(gm_dtype dtype, int64_t n, const void* a, void* out);
int gm_bv_energy_ln(gm_dtype dtype, int64_t n, const void* a, void* out);
/* accept_mask (euclidean.rs:527-533): mask[c] = log_accept[c] >= ln_u[c]
 * (NaN -> 0) */
int gm_bv_accept_mask(gm_dtype dtype, int64_t n, const void* log_accept, const void* ln_u,
                      uint8_t* mask);
/* EuclideanVector's remaining in-place ops on a [n] device vector
 * (euclidean.rs:11-60): scale_assign x = x * alpha (:396-398); fill
 * (fill_zero / zeros_like with value 0); dot = sum of a*b over all elements
 * (:400-403) into a host double (T partials, fixed order). */
int gm_bv_scale_assign(gm_dtype dtype, int64_t n, void* x, double alpha);
int gm_bv_fill(gm_dtype dtype, int64_t n, void* x, double value);
int gm_bv_dot(gm_dtype dtype, int64_t n, const void* a, const void* b, double* out);

/* A built-in target resident on the device, for logp_and_grad on device
 * buffers (BatchedHamiltonianTarget, batched_hmc.rs:18-22; hmc.rs:42-61). */
typedef struct gm_bv_target gm_bv_target;
int gm_bv_target_create(const gm_target* target, gm_dtype dtype, gm_bv_target** out);
/* grad[c,:] = d logp / d x at x[c,:]; returns logp[c] (either output may be NULL) */
int gm_bv_logp_and_grad(gm_bv_target* t, int64_t n_chains, const void* x, void* grad, void* logp);
int gm_bv_target_destroy(gm_bv_target* t);
/* One leapfrog of n_chains chains with q, p, g ([C][D]) and logp ([C],
 * nullable) in device memory, updated in place: the loop body of
 * BatchedGenericHMC::leapfrog (batched_hmc.rs:166-190) -- add_scaled_assign
 * (euclidean.rs:392-394) of the half kick, the drift, logp_and_grad
 * (hmc.rs:42-61), the second half kick -- as one kernel. Bitwise the composed
 * ops. Built-in targets, dim <= 1024. */
int gm_bv_leapfrog(gm_bv_target* t, int64_t n_chains, void* q, void* p, void* g, void* logp,
                   double step_size);

#ifdef __cplusplus
}
#endif
#endif /* GMCMC_H */
