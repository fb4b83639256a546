// gmcmc_predict.cpp — C ABI of the GLM posterior prediction (gm_glm_predict*,
// include/gmcmc.h): per data row, over all stored draws, the mean and sd of
// the linear predictor and of the mean response, the lppd and the mean and
// variance of the pointwise log-likelihood (WAIC's terms). Not in the
// reference. The kernels are in glm_predict_device.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

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

constexpr size_t PART_BUDGET = (size_t)256 << 20;  // partials of one launch pair, bytes
constexpr long long POINTWISE_CAP = 1LL << 31;     // bytes

// a device allocation of one call
struct DevMem {
  void* d = nullptr;
  ~DevMem() {
    if (d) hipFree(d);
  }
  int alloc(size_t bytes) {
    if (hipMalloc(&d, bytes ? bytes : 8) != hipSuccess) {
      d = nullptr;
      set_error("device allocation failed in the GLM prediction");
      return GM_ENOMEM;
    }
    return GM_OK;
  }
};

bool wants_ll(const gm_glm_predict_out* o) { return o->lppd || o->ll_mean || o->ll_var || o->pointwise; }

// Everything that can be refused, before any device call; build_glm's wording
// and first-offender rule for the model.
int validate(const gm_glm_desc* g, int64_t dim, gm_dtype dt, const void* draws, int64_t n_draws, int64_t stride,
             const gm_glm_predict_out* out) {
  GM_REQ(g != nullptr, "GLM predict: the model (gm_glm_desc) is NULL");
  GM_REQ(g->family == GM_GLM_BERNOULLI_LOGIT || g->family == GM_GLM_POISSON_LOG,
         "GLM target: family must be GM_GLM_BERNOULLI_LOGIT (1) or GM_GLM_POISSON_LOG (2)");
  GM_REQ(dim >= 1 && dim <= 128, "GLM target: dim must be in [1, 128]");
  GM_REQ(g->n_rows >= 1, "GLM target: n_rows must be >= 1");
  GM_REQ(g->n_rows <= (1LL << 24), "GLM target: n_rows must be <= 2^24");
  GM_REQ(g->x != nullptr, "GLM predict: x must not be NULL");
  GM_REQ(dt == GM_F32 || dt == GM_F64, "GLM predict: bad dtype");
  GM_REQ(draws != nullptr, "GLM predict: draws is NULL");
  GM_REQ(n_draws >= 1, "GLM predict: n_draws must be >= 1");
  GM_REQ(stride >= dim, "GLM predict: stride_draw must be >= dim");
  GM_REQ(out != nullptr, "GLM predict: out is NULL");
  GM_REQ(g->y != nullptr || !wants_ll(out), "GLM predict: lppd, ll_mean, ll_var and pointwise need y");
  if (out->pointwise) {
    const long long esz = dt == GM_F32 ? 4 : 8;
    GM_REQ(n_draws <= POINTWISE_CAP / (esz * g->n_rows),
           "GLM predict: the pointwise matrix (n_draws * n_rows * sizeof(dtype)) is larger than 2^31 bytes: "
           "pass the rows in blocks");
  }
  const long long N = g->n_rows, D = dim;
  auto fail = [](const std::string& m) {
    set_error(m);
    return GM_EINVAL;
  };
  for (long long n = 0; n < N; ++n) {
    for (long long j = 0; j < D; ++j)
      if (!std::isfinite(g->x[n * D + j]))
        return fail("GLM target: x is not finite at row " + std::to_string(n) + ", column " + std::to_string(j));
    if (g->y) {
      const double yn = g->y[n];
      if (!std::isfinite(yn)) return fail("GLM target: y is not finite at row " + std::to_string(n));
      if (g->family == GM_GLM_BERNOULLI_LOGIT && !(yn >= 0 && yn <= 1))
        return fail("GLM target: bernoulli_logit needs 0 <= y <= 1 at row " + std::to_string(n));
      if (g->family == GM_GLM_POISSON_LOG && !(yn >= 0))
        return fail("GLM target: poisson_log needs y >= 0 at row " + std::to_string(n));
    }
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
        gm_glm_predict_out* out) {
  struct R {
    bool on;
    ~R() {
      if (on) gm::roctx_pop();
    }
  } rr{gm::roctx_push("gm_glm_predict")};
  hipStream_t st = nullptr;
  const long long M = g->n_rows, D = dim;
  const size_t esz = dt == GM_F32 ? 4 : 8;
  const bool has_y = g->y != nullptr;
  const long long DP = 4LL * glm_predict_ksteps((int)D);
  DevMem dx, doff, dy, dc, dpart, dout, dpw;
  {
    std::vector<double> h((size_t)(M * DP), 0.0);
    for (long long n = 0; n < M; ++n)
      for (long long j = 0; j < D; ++j) h[(size_t)(n * DP + j)] = g->x[n * D + j];
    GM_TRY(upload_as(dt, h, dx));
  }
  {
    std::vector<double> h((size_t)M, 0.0);
    if (g->offset)
      for (long long n = 0; n < M; ++n) h[n] = g->offset[n];
    GM_TRY(upload_as(dt, h, doff));
    if (has_y) {
      for (long long n = 0; n < M; ++n) h[n] = g->y[n];
      GM_TRY(upload_as(dt, h, dy));
      // c_m in float64, rounded to the dtype by the upload
      for (long long n = 0; n < M; ++n) h[n] = g->family == GM_GLM_POISSON_LOG ? -std::lgamma(g->y[n] + 1.0) : 0.0;
      GM_TRY(upload_as(dt, h, dc));
    }
  }
  // rows per launch pair: whole workgroup tiles whose partials fit the budget
  const GlmPredictPlan plan = glm_predict_plan();
  const size_t per_tile = glm_predict_part_doubles(S, plan.rows) * sizeof(double);
  long long tiles = (long long)(PART_BUDGET / per_tile);
  tiles = tiles < 1 ? 1 : tiles > 32768 ? 32768 : tiles;
  long long chunk = tiles * plan.rows;
  if (chunk > M) chunk = M;
  GM_TRY(dpart.alloc(glm_predict_part_doubles(S, chunk) * sizeof(double)));
  GM_TRY(dout.alloc((size_t)7 * M * sizeof(double)));
  if (out->pointwise) GM_TRY(dpw.alloc((size_t)S * M * esz));
  for (long long r0 = 0; r0 < M; r0 += chunk) {
    GlmPredictLaunch a;
    a.x = dx.d;
    a.off = doff.d;
    a.y = dy.d;
    a.c = dc.d;
    a.draws = d_draws;
    a.S = S;
    a.stride = stride;
    a.M = M;
    a.D = (int)D;
    a.family = g->family;
    a.row0 = r0;
    a.rows = M - r0 < chunk ? M - r0 : chunk;
    a.part = (double*)dpart.d;
    a.out = (double*)dout.d;
    a.pw = dpw.d;
    GM_HIP(launch_glm_predict(dt, a, st));
  }
  std::vector<double> h((size_t)7 * M);
  GM_HIP(hipMemcpyAsync(h.data(), dout.d, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  if (out->pointwise)
    GM_HIP(hipMemcpyAsync(out->pointwise, dpw.d, (size_t)S * M * esz, hipMemcpyDeviceToHost, st));
  GM_HIP(hipStreamSynchronize(st));
  double* dst[7] = {out->eta_mean, out->eta_sd, out->mu_mean, out->mu_sd, out->lppd, out->ll_mean, out->ll_var};
  for (int k = 0; k < 7; ++k) {
    if (!dst[k]) continue;
    for (long long n = 0; n < M; ++n) dst[k][n] = h[(size_t)k * M + n];
  }
  return GM_OK;
}

}  // namespace

extern "C" {

int gm_glm_predict_device(const gm_glm_desc* model, int64_t dim, gm_dtype dtype, const void* dev_draws,
                          int64_t n_draws, int64_t stride_draw, gm_glm_predict_out* out) {
  GM_TRY(validate(model, dim, dtype, dev_draws, n_draws, stride_draw, out));
  return run(model, dim, dtype, dev_draws, n_draws, stride_draw, out);
}

int gm_glm_predict(const gm_glm_desc* model, int64_t dim, gm_dtype dtype, const void* draws, int64_t n_draws,
                   gm_glm_predict_out* out) {
  GM_TRY(validate(model, dim, dtype, draws, n_draws, dim, out));
  const size_t bytes = (size_t)n_draws * dim * (dtype == GM_F32 ? 4 : 8);
  DevMem d;
  GM_TRY(d.alloc(bytes));
  GM_HIP(hipMemcpy(d.d, draws, bytes, hipMemcpyHostToDevice));
  return run(model, dim, dtype, d.d, n_draws, dim, out);
}

int gm_glm_predict_plan(int32_t* out, int32_t cap) {
  GM_REQ(out && cap >= 0, "out is NULL or cap < 0");
  const GlmPredictPlan p = glm_predict_plan();
  const int32_t plan[3] = {p.slab, p.rows, p.tile};
  for (int i = 0; i < 3 && i < cap; ++i) out[i] = plan[i];
  return GM_OK;
}

}  // extern "C"
