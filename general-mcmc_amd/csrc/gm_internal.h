// gm_internal.h — host-side declarations shared by the C ABI (gmcmc_api.cpp)
// and the kernel translation units. Not part of the public boundary.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/gmcmc.h"
#include "gm_launch.h"

namespace gm {

void set_error(const std::string& msg);

// Device-side view of a target (pointers are device memory).
struct TargetDev {
  int kind = 0;
  int D = 0;
  double a = 1, b = 100, std = 1, norm_const = 0;
  const void* mu = nullptr;    // [D] of the sampler dtype
  const void* prec = nullptr;  // [D*D] of the sampler dtype, transposed (prec[j*D+i] = P_ij)
  const char* src = nullptr;     // CUSTOM: user source (interned, lives for the process)
  const void* params = nullptr;  // CUSTOM: [n_params] of the sampler dtype
  // GLM (glm_device.h): one device allocation of the sampler dtype,
  // iv [Dp] | y [Np] | offset [Np] | xt [Dp][Np]
  const void* glm = nullptr;
  int glm_family = 0, glm_dp = 0;
  long long glm_n = 0, glm_np = 0;
};

struct Layout {
  int lanes = 64;
  int elems = 1;
};
bool layout_supported(int lanes, int elems);
// one chain per workgroup of lanes/64 waves (HMC only, dim > 1024)
inline bool layout_is_wide(const Layout& l) { return l.lanes > 64; }
bool wide_layout_supported(int lanes, int elems, gm_dtype dt);
// largest dim of the wide path (f32; f64 is half of it)
constexpr int GM_WIDE_MAX_DIM = 16384;
Layout default_layout(int D, gm_dtype dt, int kind);
// the GLM target's own layouts and kernel entry points (glm_kernels.hip,
// glm_hmc_adapt_*.hip, glm_nuts_*.hip)
bool glm_layout_supported(int lanes, int elems);
Layout glm_default_layout(int D);
Layout nuts_wide_default(int D, gm_dtype dt);
bool nuts_wide_layout_supported(int lanes, int elems);  // nuts_wide.hip

// Events a launcher records around its kernel (either may be null).
struct LaunchEvents {
  hipEvent_t start = nullptr, stop = nullptr;
};

// An AOT kernel launch between its timing events (event records on the
// stream; hipExtLaunchKernel's in-dispatch events measured 8-14 us slower per
// call on the host, profiles/r02/launch_ab.json).
template <class... A>
hipError_t launch_timed(void (*k)(A...), dim3 grid, dim3 block, size_t lds, hipStream_t st, LaunchEvents ev,
                        A... args) {
  hipError_t e = ev.start ? hipEventRecord(ev.start, st) : hipSuccess;
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k, grid, block, lds, st, args...);
  e = hipGetLastError();
  if (e == hipSuccess && ev.stop) e = hipEventRecord(ev.stop, st);
  return e;
}
// The same events around a launch path that goes through another API (the
// runtime-compiled user-target kernels).
template <class F>
hipError_t with_events(LaunchEvents ev, hipStream_t st, F&& launch) {
  hipError_t e = ev.start ? hipEventRecord(ev.start, st) : hipSuccess;
  if (e == hipSuccess) e = launch();
  if (e == hipSuccess && ev.stop) e = hipEventRecord(ev.stop, st);
  return e;
}

// ---- HMC -------------------------------------------------------------------
hipError_t launch_hmc(gm_dtype dt, const TargetDev& tg, const Layout& lay, const HmcLaunch& a,
                      hipStream_t st, LaunchEvents ev = {});
// per-chain step sizes / diagonal metric / warm-up (hmc_adapt_kernels.hip);
// mode: 0 frozen, 1 step-size adaptation, 2 step size + Welford statistics
hipError_t launch_hmc_adapt(gm_dtype dt, const TargetDev& tg, const Layout& lay, const HmcAdaptLaunch& a,
                            int mode, hipStream_t st, LaunchEvents ev = {});
// the same kernels for the GLM target at its own layouts
hipError_t launch_glm_hmc_adapt(gm_dtype dt, const TargetDev& tg, const Layout& lay, const HmcAdaptLaunch& a, int mode,
                                hipStream_t st, LaunchEvents ev);
hipError_t launch_glm_logp_grad(gm_dtype dt, const TargetDev& tg, const Layout& lay, long long n, const void* x,
                                void* logp, void* grad, hipStream_t st);
// a warm-up window's end (rn >= 5): metric from the Welford state, restart of the dual averaging
hipError_t launch_hmc_adapt_window(gm_dtype dt, long long C, int D, double regularize, double jitter,
                                   long long rn, void* eps, const void* eps_bar, void* h_bar, void* mu,
                                   void* dinv, void* dsq, void* rmean, void* rm2, hipStream_t st);
// per-chain step sizes and one dense metric shared by all chains
// (hmc_dense_kernels.hip); mode: 0 frozen, 1 step-size adaptation
// largest dim of the dense metric (Sigma in LDS beside the target's staging;
// single-workgroup window kernel)
constexpr int GM_DENSE_MAX_DIM = 64;
hipError_t launch_hmc_dense(gm_dtype dt, const TargetDev& tg, const Layout& lay, const HmcDenseLaunch& a,
                            int mode, hipStream_t st, LaunchEvents ev = {});
// Pooled warm-up statistics in float64 (HMC dense metric, NUTS pooled metric).
// A warm-up launch stores its window rows to the slab [rows][C][D];
// pooled_accumulate then takes slab rows [0, used): the pivot c0 (mean over
// chains of row 0) when the window has no rows yet (*rn == 0), then
// s1 += sum (x - c0), S2 += sum (x - c0)(x - c0)^T row after row, in batches
// whose Gram partials fit `part` (gm_plan.h: gram_rows_for); *rn += used.
struct PooledScratch {
  void *slab = nullptr, *part = nullptr;
  size_t slab_bytes = 0, part_bytes = 0;
};
// both buffers for launches of at most `rows` window rows (ensure_buf)
int pooled_scratch_ensure(PooledScratch& ps, long long rows, long long C, int D, size_t esz);
hipError_t pooled_accumulate(gm_dtype dt, const PooledScratch& ps, long long used, long long C, int D,
                             long long* rn, double* c0, double* s1, double* S2, hipStream_t st);
// Sigma (from the statistics, or sig_in), its Cholesky factor and A = L^-T,
// float64 masters and sampler-dtype copies; statistics reset; restart of the
// dual averaging (one workgroup)
hipError_t launch_hmc_dense_window(gm_dtype dt, int D, long long C, int from_stats, long long n, double reg,
                                   double jitter, double* s1, double* S2, const double* sig_in, double* minv64,
                                   double* a64, void* minvT, void* atT, long long* counters, int count, int restart,
                                   void* eps, const void* eps_bar, void* h_bar, void* mu, hipStream_t st);

// ---- run_progress statistics (gm_track.h, tracker_kernels.hip) -------------
// ChainTracker::new for every chain from the current positions
hipError_t launch_ct_init(gm_dtype dt, long long C, int D, const void* q, const TrackLaunch& t,
                          hipStream_t st);
// ChainTracker::stats of every chain + collect_rhat (stats.rs:122-193) -> rhat[D],
// and the mean acceptance EMA over chains -> p_mean[0]
hipError_t launch_ct_rhat(long long C, int D, unsigned long long n, const TrackLaunch& t, float* rhat,
                          float* p_mean, hipStream_t st);
// MultiChainTracker::step / rhat (stats.rs:199-339) on [C][P] positions
hipError_t launch_mct_step(gm_dtype dt, long long C, int P, const void* x, float* mean, float* msq,
                           float* last, int* flags, float* p_accept, unsigned long long n_after,
                           hipStream_t st);
hipError_t launch_mct_rhat(long long C, int P, unsigned long long n, const float* mean, const float* msq,
                           float* rhat, hipStream_t st);

// ---- per-transition sampler statistics (stats_kernels.hip) -------------------
// The reduction of record rows [r0, r0 + rows) of rec [.][C] (StatsRec of the
// dtype): out [GM_STATS_FIELDS][C] and the chains' totals tot
// [GM_STATS_FIELDS] (include/gmcmc.h), float64 on the device; scratch:
// stats_reduce_scratch_bytes(C, rows) bytes. max_depth 0: nothing counts as
// having reached it (HMC).
size_t stats_reduce_scratch_bytes(long long C, long long rows);
hipError_t launch_stats_reduce(gm_dtype dt, const void* rec, long long C, long long r0, long long rows,
                               int max_depth, double* scratch, double* out, double* tot, hipStream_t st);

// ---- MH --------------------------------------------------------------------
hipError_t launch_mh(gm_dtype dt, const TargetDev& tg, const Layout& lay, const MhLaunch& a,
                     hipStream_t st, LaunchEvents ev = {});
// per-chain proposal scale / diagonal shape / warm-up (mh_adapt_kernels.hip);
// mode: 0 frozen, 1 scale adaptation, 2 scale + Welford statistics
hipError_t launch_mh_adapt(gm_dtype dt, const TargetDev& tg, const Layout& lay, const MhAdaptLaunch& a, int mode,
                           hipStream_t st, LaunchEvents ev = {});
// a warm-up window's end (rn >= 5): shape from the Welford state, restart of the dual averaging
hipError_t launch_mh_adapt_window(gm_dtype dt, long long C, int D, double regularize, double jitter, long long rn,
                                  void* scale, const void* scale_bar, void* h_bar, void* mu, void* diag,
                                  void* rmean, void* rm2, hipStream_t st);

// ---- target evaluation -----------------------------------------------------
// one leapfrog of n chains, state in HBM (util_device.h leapfrog_hbm_kernel)
hipError_t launch_leapfrog_hbm(gm_dtype dt, const TargetDev& tg, const Layout& lay, long long n, void* q,
                               void* p, void* g, void* logp, double eps, hipStream_t st);
hipError_t launch_logp_grad(gm_dtype dt, const TargetDev& tg, const Layout& lay, long long n,
                            const void* x, void* logp, void* grad, hipStream_t st);

// ---- granular BatchVector ops (bv_kernels.hip) -------------------------------
hipError_t launch_bv_kinetic(gm_dtype dt, const Layout& lay, long long C, int D, const void* p, void* ke,
                             hipStream_t st);
hipError_t launch_bv_masked_assign(gm_dtype dt, long long C, int D, void* x, const void* o,
                                   const uint8_t* mask, hipStream_t st);
hipError_t launch_bv_axpy(gm_dtype dt, long long n, void* x, const void* o, double alpha, hipStream_t st);
hipError_t launch_bv_scale(gm_dtype dt, long long n, void* x, double alpha, hipStream_t st);
hipError_t launch_bv_fill(gm_dtype dt, long long n, void* x, double v, hipStream_t st);
hipError_t launch_bv_dot(gm_dtype dt, long long n, const void* a, const void* b, double* out, hipStream_t st);
hipError_t launch_bv_normal(gm_dtype dt, long long C, int D, void* out, uint64_t seed, uint32_t off,
                            uint64_t step, uint32_t tag, hipStream_t st);
hipError_t launch_bv_uniform(gm_dtype dt, long long C, void* out, uint64_t seed, uint32_t off, uint64_t step,
                             uint32_t tag, hipStream_t st);
hipError_t launch_bv_energy(gm_dtype dt, int op, long long n, const void* a, const void* b, void* out,
                            hipStream_t st);
hipError_t launch_bv_accept(gm_dtype dt, long long n, const void* la, const void* lnu, uint8_t* mask,
                            hipStream_t st);

// target construction (gmcmc_api.cpp): device copies of mean / precision
int build_target(const gm_target* t, gm_dtype dt, long long dim, TargetDev* out, void** d_mu,
                 void** d_prec);

// ---- utilities -------------------------------------------------------------
// A grow-only device buffer: at least `need` bytes behind *p (gmcmc_api.cpp);
// GM_ENOMEM with the error text set when the allocation fails.
int ensure_buf(void** p, size_t* cap, size_t need);
// [rows][C][D] -> [C][rows][D]
// dst = src in 16-byte words (both 16-byte aligned), util_kernels.hip
hipError_t launch_copy16(const void* src, void* dst, long long words, hipStream_t st);
hipError_t launch_transpose_samples(gm_dtype dt, const void* src, void* dst, long long rows,
                                    long long C, long long D, hipStream_t st);

// roctx ranges when GMCMC_ROCTX=1 and the roctx library can be opened
// (gmcmc_api.cpp); push returns whether a range was opened
bool roctx_push(const char* name);
void roctx_pop();

}  // namespace gm
