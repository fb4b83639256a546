// gmcmc_loo.cpp — C ABI of the GLM PSIS-LOO (gm_glm_loo*, include/gmcmc.h):
// per data row, over all stored draws, the Pareto-smoothed leave-one-out elpd
// and the Pareto shape k. Not in the reference. The kernels are in
// glm_loo_device.h; the lppd is gm_glm_predict's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "glm_loo.h"
#include "glm_predict.h"
#include "gm_internal.h"

using namespace gm;

#define GM_REQ(cond, msg) \
  do {                    \
    if (!(cond)) {        \
      set_error(msg);     \
      return GM_EINVAL;   \
    }                     \
  } while (0)
#define GM_HIP(expr)                                                               \
  do {                                                                             \
    hipError_t _e = (expr);                                                        \
    if (_e != hipSuccess) {                                                        \
      set_error(std::string("HIP error ") + hipGetErrorString(_e) + " at " #expr); \
      return GM_EHIP;                                                              \
    }                                                                              \
  } while (0)
#define GM_TRY(expr)     \
  do {                   \
    int _rc = (expr);    \
    if (_rc) return _rc; \
  } while (0)

namespace {

// bytes, 4.25 GiB: 64 rows of 2^24 draws in f32; 256 rows (a row workgroup for every compute unit) of
// 4096 chains x 1000 draws in f32, 128 in f64
constexpr long long DEFAULT_WORKSPACE = (1LL << 32) + (1LL << 28);
constexpr long long GROUP_ROWS = 64;                // rows come in multiples of the product kernel's tile
constexpr long long MAX_GROUP = 1LL << 20;          // rows per group at most (the launcher's grid)

// a device allocation of one call
struct DevMem {
  void* d = nullptr;
  ~DevMem() {
    if (d) hipFree(d);
  }
  int alloc(size_t bytes) {
    if (hipMalloc(&d, bytes ? bytes : 8) != hipSuccess) {
      d = nullptr;
      set_error("device allocation failed in the GLM PSIS-LOO");
      return GM_ENOMEM;
    }
    return GM_OK;
  }
};

// the split of one call: a function of (dtype, n_draws, n_rows, reff, workspace_bytes) only
struct Plan {
  long long tail_len, P, ld, per_row, rows, workspace, used, max_draws;
};

// tail length, sort slots, row stride and workspace bytes of one row of S draws
void row_sizes(gm_dtype dt, long long S, double reff, Plan& p) {
  const double a = std::floor(0.2 * (double)S), b = std::ceil(3.0 * std::sqrt((double)S / reff));
  p.tail_len = (long long)(a < b ? a : b);
  p.P = 1;
  while (p.P < p.tail_len + 1) p.P <<= 1;
  p.ld = (S + 3) / 4 * 4;
  const long long esz = dt == GM_F32 ? 4 : 8;
  // ll [ld] of dtype, the sort slots and their exponentials [P] float64 each, bad, elpd_loo, pareto_k
  p.per_row = p.ld * esz + 2 * p.P * 8 + 4 + 16;
}

// the largest n_draws <= 2^24 of which the workspace holds 64 rows (0: none); the row's bytes grow with S
long long largest_draws(gm_dtype dt, double reff, long long workspace) {
  long long lo = 0, hi = glm_loo_max_draws();
  while (lo < hi) {
    const long long mid = lo + (hi - lo + 1) / 2;
    Plan q;
    row_sizes(dt, mid, reff, q);
    if (GROUP_ROWS * q.per_row <= workspace)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

int make_plan(gm_dtype dt, int64_t S, int64_t N, double reff, int64_t workspace, Plan& p) {
  GM_REQ(dt == GM_F32 || dt == GM_F64, "GLM loo: bad dtype");
  GM_REQ(S >= 1, "GLM loo: n_draws must be >= 1");
  GM_REQ(S <= glm_loo_max_draws(), "GLM loo: n_draws must be <= 2^24");
  GM_REQ(N >= 1, "GLM target: n_rows must be >= 1");
  GM_REQ(N <= (1LL << 24), "GLM target: n_rows must be <= 2^24");
  GM_REQ(std::isfinite(reff) && reff > 0.0, "GLM loo: reff must be finite and > 0");
  GM_REQ(workspace >= 0, "GLM loo: workspace_bytes must be >= 0 (0: the default)");
  row_sizes(dt, S, reff, p);
  p.workspace = workspace ? workspace : DEFAULT_WORKSPACE;
  p.max_draws = largest_draws(dt, reff, p.workspace);
  long long rows = p.workspace / p.per_row / GROUP_ROWS * GROUP_ROWS;
  if (rows < GROUP_ROWS) {
    set_error("GLM loo: workspace_bytes = " + std::to_string(p.workspace) + " is too small: " +
              std::to_string(GROUP_ROWS) + " rows of " + std::to_string(S) + " draws need " +
              std::to_string(GROUP_ROWS * p.per_row) + " bytes (it holds them for up to " +
              std::to_string(p.max_draws) + " draws)");
    return GM_EINVAL;
  }
  const long long n_pad = (N + GROUP_ROWS - 1) / GROUP_ROWS * GROUP_ROWS;
  rows = rows > n_pad ? n_pad : rows;
  p.rows = rows > MAX_GROUP ? MAX_GROUP : rows;
  p.used = p.rows * p.per_row;
  return GM_OK;
}

// Everything that can be refused, before any device call; build_glm's wording
// and first-offender rule for the model (as gm_glm_predict).
int validate(const gm_glm_desc* g, int64_t dim, gm_dtype dt, const void* draws, int64_t n_draws, int64_t stride,
             double reff, int64_t workspace, const gm_glm_loo_out* out, Plan& plan) {
  GM_REQ(g != nullptr, "GLM loo: the model (gm_glm_desc) is NULL");
  GM_REQ(g->family == GM_GLM_BERNOULLI_LOGIT || g->family == GM_GLM_POISSON_LOG,
         "GLM target: family must be GM_GLM_BERNOULLI_LOGIT (1) or GM_GLM_POISSON_LOG (2)");
  GM_REQ(dim >= 1 && dim <= 128, "GLM target: dim must be in [1, 128]");
  GM_REQ(g->n_rows >= 1, "GLM target: n_rows must be >= 1");
  GM_REQ(g->n_rows <= (1LL << 24), "GLM target: n_rows must be <= 2^24");
  GM_REQ(g->x != nullptr, "GLM loo: x must not be NULL");
  GM_REQ(g->y != nullptr, "GLM loo: y must not be NULL");
  GM_REQ(dt == GM_F32 || dt == GM_F64, "GLM loo: bad dtype");
  GM_REQ(draws != nullptr, "GLM loo: draws is NULL");
  GM_REQ(n_draws >= 1, "GLM loo: n_draws must be >= 1");
  GM_REQ(stride >= dim, "GLM loo: stride_draw must be >= dim");
  GM_REQ(out != nullptr, "GLM loo: out is NULL");
  GM_TRY(make_plan(dt, n_draws, g->n_rows, reff, workspace, plan));
  const long long N = g->n_rows, D = dim;
  auto fail = [](const std::string& m) {
    set_error(m);
    return GM_EINVAL;
  };
  for (long long n = 0; n < N; ++n) {
    for (long long j = 0; j < D; ++j)
      if (!std::isfinite(g->x[n * D + j]))
        return fail("GLM target: x is not finite at row " + std::to_string(n) + ", column " + std::to_string(j));
    const double yn = g->y[n];
    if (!std::isfinite(yn)) return fail("GLM target: y is not finite at row " + std::to_string(n));
    if (g->family == GM_GLM_BERNOULLI_LOGIT && !(yn >= 0 && yn <= 1))
      return fail("GLM target: bernoulli_logit needs 0 <= y <= 1 at row " + std::to_string(n));
    if (g->family == GM_GLM_POISSON_LOG && !(yn >= 0))
      return fail("GLM target: poisson_log needs y >= 0 at row " + std::to_string(n));
    if (g->offset && !std::isfinite(g->offset[n]))
      return fail("GLM target: offset is not finite at row " + std::to_string(n));
  }
  return GM_OK;
}

template <class T> int upload(const std::vector<double>& h, DevMem& d) {
  std::vector<T> t(h.size());
  for (size_t i = 0; i < h.size(); ++i) t[i] = (T)h[i];
  GM_TRY(d.alloc(t.size() * sizeof(T)));
  GM_HIP(hipMemcpy(d.d, t.data(), t.size() * sizeof(T), hipMemcpyHostToDevice));
  return GM_OK;
}
int upload_as(gm_dtype dt, const std::vector<double>& h, DevMem& d) {
  return dt == GM_F32 ? upload<float>(h, d) : upload<double>(h, d);
}

int run(const gm_glm_desc* g, int64_t dim, gm_dtype dt, const void* d_draws, int64_t S, int64_t stride,
        const Plan& plan, gm_glm_loo_out* out) {
  struct R {
    bool on;
    ~R() {
      if (on) gm::roctx_pop();
    }
  } rr{gm::roctx_push("gm_glm_loo")};
  hipStream_t st = nullptr;
  const long long N = g->n_rows, D = dim;
  const size_t esz = dt == GM_F32 ? 4 : 8;
  const long long DP = 4LL * glm_predict_ksteps((int)D);
  DevMem dx, doff, dy, dc, dll, dsort, deb, dbad, dout;
  {
    std::vector<double> h((size_t)(N * DP), 0.0);
    for (long long n = 0; n < N; ++n)
      for (long long j = 0; j < D; ++j) h[(size_t)(n * DP + j)] = g->x[n * D + j];
    GM_TRY(upload_as(dt, h, dx));
  }
  {
    std::vector<double> h((size_t)N, 0.0);
    if (g->offset)
      for (long long n = 0; n < N; ++n) h[n] = g->offset[n];
    GM_TRY(upload_as(dt, h, doff));
    for (long long n = 0; n < N; ++n) h[n] = g->y[n];
    GM_TRY(upload_as(dt, h, dy));
    // c_m in float64, rounded to the dtype by the upload (as gm_glm_predict)
    for (long long n = 0; n < N; ++n) h[n] = g->family == GM_GLM_POISSON_LOG ? -std::lgamma(g->y[n] + 1.0) : 0.0;
    GM_TRY(upload_as(dt, h, dc));
  }
  const long long R = plan.rows, M = plan.tail_len, P = plan.P;
  GM_TRY(dll.alloc((size_t)R * plan.ld * esz));
  GM_TRY(dsort.alloc((size_t)R * P * sizeof(double)));
  GM_TRY(deb.alloc((size_t)R * P * sizeof(double)));
  GM_TRY(dbad.alloc((size_t)R * sizeof(int)));
  GM_TRY(dout.alloc((size_t)2 * R * sizeof(double)));
  std::vector<double> h((size_t)2 * R);
  std::vector<int> hbad((size_t)R);
  long long n_bad = 0;
  for (long long r0 = 0; r0 < N; r0 += R) {
    GlmLooLaunch a;
    a.x = dx.d;
    a.off = doff.d;
    a.y = dy.d;
    a.c = dc.d;
    a.draws = d_draws;
    a.S = S;
    a.stride = stride;
    a.M = N;
    a.D = (int)D;
    a.family = g->family;
    a.row0 = r0;
    a.rows = N - r0 < R ? N - r0 : R;
    a.ll = dll.d;
    a.ld = plan.ld;
    a.bad = (int*)dbad.d;
    a.tail_len = M;
    a.P = P;
    a.sortb = (double*)dsort.d;
    a.eb = (double*)deb.d;
    a.out = (double*)dout.d;
    GM_HIP(launch_glm_loo(dt, a, st));
    GM_HIP(hipMemcpyAsync(h.data(), dout.d, (size_t)2 * a.rows * sizeof(double), hipMemcpyDeviceToHost, st));
    GM_HIP(hipMemcpyAsync(hbad.data(), dbad.d, (size_t)a.rows * sizeof(int), hipMemcpyDeviceToHost, st));
    if (out->tail && M > 0)  // slots 1 .. M of every row
      GM_HIP(hipMemcpy2DAsync(out->tail + r0 * M, (size_t)M * sizeof(double), (const double*)dsort.d + 1,
                              (size_t)P * sizeof(double), (size_t)M * sizeof(double), (size_t)a.rows,
                              hipMemcpyDeviceToHost, st));
    GM_HIP(hipStreamSynchronize(st));
    for (long long n = 0; n < a.rows; ++n) {
      if (out->elpd_loo) out->elpd_loo[r0 + n] = h[(size_t)n];
      if (out->pareto_k) out->pareto_k[r0 + n] = h[(size_t)(a.rows + n)];
      n_bad += hbad[(size_t)n] != 0;
    }
  }
  out->tail_len = M;
  out->n_nonfinite = n_bad;
  return GM_OK;
}

}  // namespace

extern "C" {

int gm_glm_loo_device(const gm_glm_desc* model, int64_t dim, gm_dtype dtype, const void* dev_draws, int64_t n_draws,
                      int64_t stride_draw, double reff, int64_t workspace_bytes, gm_glm_loo_out* out) {
  Plan plan;
  GM_TRY(validate(model, dim, dtype, dev_draws, n_draws, stride_draw, reff, workspace_bytes, out, plan));
  return run(model, dim, dtype, dev_draws, n_draws, stride_draw, plan, out);
}

int gm_glm_loo(const gm_glm_desc* model, int64_t dim, gm_dtype dtype, const void* draws, int64_t n_draws, double reff,
               int64_t workspace_bytes, gm_glm_loo_out* out) {
  Plan plan;
  GM_TRY(validate(model, dim, dtype, draws, n_draws, dim, reff, workspace_bytes, out, plan));
  const size_t bytes = (size_t)n_draws * dim * (dtype == GM_F32 ? 4 : 8);
  DevMem d;
  GM_TRY(d.alloc(bytes));
  GM_HIP(hipMemcpy(d.d, draws, bytes, hipMemcpyHostToDevice));
  return run(model, dim, dtype, d.d, n_draws, dim, plan, out);
}

int gm_glm_loo_plan(gm_dtype dtype, int64_t n_draws, int64_t n_rows, double reff, int64_t workspace_bytes,
                    int64_t* out, int32_t cap) {
  GM_REQ(out && cap >= 0, "out is NULL or cap < 0");
  Plan p;
  GM_TRY(make_plan(dtype, n_draws, n_rows, reff, workspace_bytes, p));
  const int64_t v[7] = {p.tail_len, p.rows, p.used, p.per_row, DEFAULT_WORKSPACE, p.max_draws, p.P};
  for (int i = 0; i < 7 && i < cap; ++i) out[i] = v[i];
  return GM_OK;
}

}  // extern "C"
