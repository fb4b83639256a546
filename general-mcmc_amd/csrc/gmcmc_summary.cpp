// gmcmc_summary.cpp — C ABI of the posterior summary (gm_summary*,
// gm_rank_normalize; include/gmcmc.h): rank-normalised split-R-hat, bulk and
// tail ESS (Vehtari et al. 2021), quantiles, pooled mean / sd. Not in the
// reference. The stages are in summary_kernels.hip; the four Appendix-B passes
// per parameter (z, z_fold, I05, I95) are diag_series + diag_final as they are.
#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>
#include <map>
#include <string>
#include <vector>

#include "gm_diag.h"
#include "gm_summary.h"

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
#define GM_TRY(expr)       \
  do {                     \
    int _rc = (expr);      \
    if (_rc) return _rc;   \
  } while (0)

namespace {
// Device buffers of the summary, kept per (host thread, device) and only
// grown, as the diagnostics' are (gmcmc_diag.cpp). Never freed.
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  int alloc(size_t n) {
    if (n == 0) n = 8;
    if (cap >= n) return GM_OK;
    if (p) hipFree(p);
    p = nullptr;
    cap = 0;
    if (hipMalloc(&p, n) != hipSuccess) {
      p = nullptr;
      set_error("device allocation failed in the posterior summary");
      return GM_ENOMEM;
    }
    cap = n;
    return GM_OK;
  }
};
struct SumBufs {
  DevBuf ka, kb, ia, ib, hist, series, part, ostat, probs;  // one chunk
  DevBuf cm, s2, ac;                                        // diag_series products of one chunk
  DevBuf mean, sdev, quant, diag, flags;                    // results, [P]
  DiagScratch ws;
};
SumBufs& sum_bufs() {
  static thread_local std::map<int, SumBufs*> per_device;
  int dev = 0;
  hipGetDevice(&dev);
  SumBufs*& b = per_device[dev];
  if (!b) b = new SumBufs();
  return *b;
}

constexpr size_t CHUNK_BYTES = (size_t)1 << 30;  // scratch budget of one chunk of parameters
constexpr int MAX_PROBS = 32;

int validate(const void* sample, gm_dtype dtype, int64_t C, int64_t N, int64_t P) {
  GM_REQ(dtype == GM_F32 || dtype == GM_F64, "bad dtype");
  GM_REQ(sample, "sample is NULL");
  GM_REQ(C >= 1 && N >= 4 && P >= 1, "need n_chains >= 1, n_draws >= 4, n_params >= 1");
  GM_REQ(C < ((int64_t)1 << 31) && N < ((int64_t)1 << 32) && 2 * C * (N / 2) < ((int64_t)1 << 31),
         "the pooled split draws of one parameter (2 * n_chains * (n_draws / 2)) must number less than 2^31");
  return GM_OK;
}
int validate_probs(int32_t n_probs, const double* probs, const gm_summary_out* out) {
  GM_REQ(out, "out is NULL");
  GM_REQ(n_probs >= 0 && n_probs <= MAX_PROBS, "n_probs must be in [0, 32]");
  GM_REQ(n_probs == 0 || probs, "probs is NULL");
  for (int j = 0; j < n_probs; ++j) GM_REQ(probs[j] >= 0.0 && probs[j] <= 1.0, "every prob must be in [0, 1]");
  return GM_OK;
}

// rank mode (d_ranks or d_z not null): only the ranks / normal scores, of Y or
// (folded) of |Y - median|, to device [C][N][P] f64. Otherwise the summary.
int run(const void* x, gm_dtype dt, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sd, int64_t sp,
        int n_probs, const double* probs, gm_summary_out* out, bool rank_mode, bool folded, double* d_ranks,
        double* d_z) {
  struct R {
    bool on;
    ~R() {
      if (on) gm::roctx_pop();
    }
  } rr{gm::roctx_push(rank_mode ? "gm_rank_normalize" : "gm_summary")};
  hipStream_t st = nullptr;
  SmShape s;
  s.C = C;
  s.N = N;
  s.h = (int)(N / 2);
  s.M = 2 * C * s.h;
  const int kbytes = dt == GM_F32 ? 4 : 8;
  const size_t hist_w = sm_hist_words(s.M);
  const size_t per_param = (size_t)s.M * 24 + (size_t)C * N * 4 + hist_w * 4;
  int PC = (int)(CHUNK_BYTES / per_param);
  PC = PC < 1 ? 1 : PC > SM_PC_MAX ? SM_PC_MAX : PC;
  if (PC > 8) PC -= PC % 8;  // whole parameter tiles (8) for diag_series' kernels
  if (PC > P) PC = (int)P;
  // host-side order-statistic indices (f64, as the definition states)
  const long long k05 = (long long)std::floor((double)(s.M - 1) * 0.05);
  const long long k95 = (long long)std::floor((double)(s.M - 1) * 0.95);

  SumBufs& B = sum_bufs();
  GM_TRY(B.ka.alloc((size_t)s.M * 8 * PC));
  GM_TRY(B.kb.alloc((size_t)s.M * 8 * PC));
  GM_TRY(B.ia.alloc((size_t)s.M * 4 * PC));
  GM_TRY(B.ib.alloc((size_t)s.M * 4 * PC));
  GM_TRY(B.hist.alloc(hist_w * 4 * PC));
  GM_TRY(B.ostat.alloc(sizeof(double) * 3 * PC));
  GM_TRY(B.probs.alloc(sizeof(double) * MAX_PROBS));
  GM_TRY(B.quant.alloc(sizeof(double) * (size_t)(n_probs > 0 ? n_probs : 1) * P));
  GM_TRY(B.flags.alloc(sizeof(int) * P));
  if (!rank_mode) {
    GM_TRY(B.series.alloc((size_t)C * N * 4 * PC));
    GM_TRY(B.part.alloc(sm_moment_words(C, N) * sizeof(double)));
    GM_TRY(B.cm.alloc(sizeof(double) * 2 * C * PC));
    GM_TRY(B.s2.alloc(sizeof(double) * 2 * C * PC));
    GM_TRY(B.ac.alloc(sizeof(double) * s.h * PC));
    GM_TRY(B.mean.alloc(sizeof(double) * P));
    GM_TRY(B.sdev.alloc(sizeof(double) * P));
    GM_TRY(B.diag.alloc(sizeof(float) * 8 * P));
  }
  uint32_t *ia = (uint32_t*)B.ia.p, *ib = (uint32_t*)B.ib.p, *hist = (uint32_t*)B.hist.p;
  int* flags = (int*)B.flags.p;
  double *ostat = (double*)B.ostat.p, *quant = (double*)B.quant.p, *dprobs = (double*)B.probs.p;
  float *series = (float*)B.series.p, *diag = (float*)B.diag.p;
  GM_HIP(hipMemsetAsync(flags, 0, sizeof(int) * P, st));
  if (n_probs > 0) GM_HIP(hipMemcpyAsync(dprobs, probs, sizeof(double) * n_probs, hipMemcpyHostToDevice, st));

  for (int64_t p0 = 0; p0 < P; p0 += PC) {
    const int pc = (int)(P - p0 < PC ? P - p0 : PC);
    // Appendix B of the series buffer -> slot (0 z, 1 z_fold, 2 I05, 3 I95) of diag: [4][2][P]
    auto appb = [&](int slot) -> int {
      GM_TRY(diag_series(GM_F32, series, C, N, pc, N * pc, pc, 1, (double*)B.cm.p, (double*)B.s2.p, (double*)B.ac.p,
                         B.ws, st));
      return diag_final((double*)B.cm.p, (double*)B.s2.p, (double*)B.ac.p, 2 * C, 1, s.h, pc,
                        diag + (size_t)(2 * slot) * P + p0, diag + (size_t)(2 * slot + 1) * P + p0, st);
    };
    if (!rank_mode)
      GM_TRY(sm_moments(dt, x, C, N, sc, sd, sp, p0, pc, (double*)B.part.p, (double*)B.mean.p + p0,
                        (double*)B.sdev.p + p0, st));
    GM_TRY(sm_extract(dt, x, s, sc, sd, sp, p0, pc, B.ka.p, ia, flags + p0, st));
    GM_TRY(sm_sort(kbytes, B.ka.p, B.kb.p, ia, ib, hist, s.M, pc, st));
    GM_TRY(sm_order(kbytes, B.ka.p, s.M, pc, k05, k95, rank_mode ? 0 : n_probs, dprobs, ostat, quant + p0, P,
                    flags + p0, st));
    if (!rank_mode) {
      GM_TRY(sm_tie(kbytes, B.ka.p, ia, s, pc, series, nullptr, nullptr, N * pc, pc, st));
      GM_TRY(appb(0));
      GM_TRY(sm_indicator(kbytes, B.ka.p, ia, s, pc, k05, series, st));
      GM_TRY(appb(2));
      GM_TRY(sm_indicator(kbytes, B.ka.p, ia, s, pc, k95, series, st));
      GM_TRY(appb(3));
    } else if (!folded) {
      GM_TRY(sm_tie(kbytes, B.ka.p, ia, s, pc, nullptr, d_ranks ? d_ranks + p0 : nullptr, d_z ? d_z + p0 : nullptr,
                    N * P, P, st));
    }
    if (!rank_mode || folded) {
      // |Y - median| as 8-byte keys into (kb, ib), sorted there with (ka, ia) as the other half
      GM_TRY(sm_fold(kbytes, B.ka.p, ia, s.M, pc, ostat, B.kb.p, ib, st));
      GM_TRY(sm_sort(8, B.kb.p, B.ka.p, ib, ia, hist, s.M, pc, st));
      if (rank_mode) {
        GM_TRY(sm_tie(8, B.kb.p, ib, s, pc, nullptr, d_ranks ? d_ranks + p0 : nullptr, d_z ? d_z + p0 : nullptr,
                      N * P, P, st));
      } else {
        GM_TRY(sm_tie(8, B.kb.p, ib, s, pc, series, nullptr, nullptr, N * pc, pc, st));
        GM_TRY(appb(1));
      }
    }
  }
  if (rank_mode) {
    GM_HIP(hipStreamSynchronize(st));
    return GM_OK;
  }
  // the results: one copy each and the call's only synchronisation
  std::vector<double> mean(P), sdev(P), q((size_t)n_probs * P);
  std::vector<float> dg((size_t)8 * P);
  std::vector<int> fl(P);
  GM_HIP(hipMemcpyAsync(mean.data(), B.mean.p, sizeof(double) * P, hipMemcpyDeviceToHost, st));
  GM_HIP(hipMemcpyAsync(sdev.data(), B.sdev.p, sizeof(double) * P, hipMemcpyDeviceToHost, st));
  if (n_probs > 0)
    GM_HIP(hipMemcpyAsync(q.data(), quant, sizeof(double) * n_probs * P, hipMemcpyDeviceToHost, st));
  GM_HIP(hipMemcpyAsync(dg.data(), diag, sizeof(float) * 8 * P, hipMemcpyDeviceToHost, st));
  GM_HIP(hipMemcpyAsync(fl.data(), flags, sizeof(int) * P, hipMemcpyDeviceToHost, st));
  GM_HIP(hipStreamSynchronize(st));
  const double nan = std::numeric_limits<double>::quiet_NaN();
  auto at = [&](int slot, int ess, int64_t p) { return (double)dg[(size_t)(2 * slot + ess) * P + p]; };
  // NaN-propagating max / min
  auto nmax = [&](double a, double b) { return std::isnan(a) || std::isnan(b) ? nan : a > b ? a : b; };
  auto nmin = [&](double a, double b) { return std::isnan(a) || std::isnan(b) ? nan : a < b ? a : b; };
  for (int64_t p = 0; p < P; ++p) {
    const bool bad = fl[p] & 1, flat = fl[p] & 2;
    if (out->mean) out->mean[p] = bad ? nan : mean[p];
    if (out->sd) out->sd[p] = bad ? nan : sdev[p];
    if (out->quantiles)
      for (int j = 0; j < n_probs; ++j) out->quantiles[(size_t)j * P + p] = bad ? nan : q[(size_t)j * P + p];
    const bool none = bad || flat;
    if (out->rhat) out->rhat[p] = none ? nan : nmax(1.0 / at(0, 0, p), 1.0 / at(1, 0, p));
    if (out->ess_bulk) out->ess_bulk[p] = none ? nan : at(0, 1, p);
    if (out->ess_tail) out->ess_tail[p] = none ? nan : nmin(at(2, 1, p), at(3, 1, p));
  }
  return GM_OK;
}

// a host [C][N][P] sample's device copy, for one call
struct DevCopy {
  void* d = nullptr;
  ~DevCopy() {
    if (d) hipFree(d);
  }
  int alloc(size_t bytes) {
    if (hipMalloc(&d, bytes) != hipSuccess) {
      d = nullptr;
      set_error("device allocation failed in the posterior summary");
      return GM_ENOMEM;
    }
    return GM_OK;
  }
};
}  // namespace

extern "C" {

int gm_summary_device(const void* dev_sample, gm_dtype dtype, int64_t n_chains, int64_t n_draws, int64_t n_params,
                      int64_t stride_chain, int64_t stride_draw, int64_t stride_param, int32_t n_probs,
                      const double* probs, gm_summary_out* out) {
  GM_TRY(validate(dev_sample, dtype, n_chains, n_draws, n_params));
  GM_TRY(validate_probs(n_probs, probs, out));
  return run(dev_sample, dtype, n_chains, n_draws, n_params, stride_chain, stride_draw, stride_param, n_probs, probs,
             out, false, false, nullptr, nullptr);
}

int gm_summary(const void* sample, gm_dtype dtype, int64_t n_chains, int64_t n_draws, int64_t n_params,
               int32_t n_probs, const double* probs, gm_summary_out* out) {
  GM_TRY(validate(sample, dtype, n_chains, n_draws, n_params));
  GM_TRY(validate_probs(n_probs, probs, out));
  const size_t bytes = (size_t)n_chains * n_draws * n_params * (dtype == GM_F32 ? 4 : 8);
  DevCopy d;
  GM_TRY(d.alloc(bytes));
  GM_HIP(hipMemcpy(d.d, sample, bytes, hipMemcpyHostToDevice));
  return run(d.d, dtype, n_chains, n_draws, n_params, n_draws * n_params, n_params, 1, n_probs, probs, out, false,
             false, nullptr, nullptr);
}

int gm_rank_normalize(const void* sample, gm_dtype dtype, int64_t n_chains, int64_t n_draws, int64_t n_params,
                      int32_t folded, double* ranks_out, double* z_out) {
  GM_TRY(validate(sample, dtype, n_chains, n_draws, n_params));
  if (!ranks_out && !z_out) return GM_OK;
  const size_t n = (size_t)n_chains * n_draws * n_params;
  DevCopy d, r, z;
  GM_TRY(d.alloc(n * (dtype == GM_F32 ? 4 : 8)));
  GM_HIP(hipMemcpy(d.d, sample, n * (dtype == GM_F32 ? 4 : 8), hipMemcpyHostToDevice));
  // all-ones bytes are a NaN: what an odd N's middle draw keeps
  if (ranks_out) {
    GM_TRY(r.alloc(n * 8));
    GM_HIP(hipMemset(r.d, 0xff, n * 8));
  }
  if (z_out) {
    GM_TRY(z.alloc(n * 8));
    GM_HIP(hipMemset(z.d, 0xff, n * 8));
  }
  GM_TRY(run(d.d, dtype, n_chains, n_draws, n_params, n_draws * n_params, n_params, 1, 0, nullptr, nullptr, true,
             folded != 0, (double*)r.d, (double*)z.d));
  if (ranks_out) GM_HIP(hipMemcpy(ranks_out, r.d, n * 8, hipMemcpyDeviceToHost));
  if (z_out) GM_HIP(hipMemcpy(z_out, z.d, n * 8, hipMemcpyDeviceToHost));
  return GM_OK;
}

int gm_summary_sort_plan(int32_t* out, int32_t cap) {
  GM_REQ(out && cap >= 0, "out is NULL or cap < 0");
  const int32_t plan[4] = {SM_LDS_MAX, SM_TILE, SM_RADIX_BITS, SM_PC_MAX};
  for (int i = 0; i < 4 && i < cap; ++i) out[i] = plan[i];
  return GM_OK;
}

}  // extern "C"
