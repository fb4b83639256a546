// hmc_adapt_kernels.hip — launchers of hmc_adapt_kernel (hmc_adapt_device.h:
// HMC with per-chain step sizes and a per-chain diagonal metric, and their
// warm-up) and the window-end update that runs between two of its launches.
// The kernel's instantiations are in hmc_adapt_{f32,f64}_m{0,1,2}.hip.
#include "gm_jit.h"
#include "gm_rng.h"

namespace gm {

#define GM_HA_DECL(N) \
  hipError_t N(const TargetDev&, const Layout&, const HmcAdaptLaunch&, hipStream_t, LaunchEvents);
GM_HA_DECL(launch_hmc_adapt_f32_m0)
GM_HA_DECL(launch_hmc_adapt_f32_m1)
GM_HA_DECL(launch_hmc_adapt_f32_m2)
GM_HA_DECL(launch_hmc_adapt_f64_m0)
GM_HA_DECL(launch_hmc_adapt_f64_m1)
GM_HA_DECL(launch_hmc_adapt_f64_m2)
#undef GM_HA_DECL

hipError_t launch_hmc_adapt(gm_dtype dt, const TargetDev& tg, const Layout& lay, const HmcAdaptLaunch& a,
                            int mode, hipStream_t st, LaunchEvents ev) {
  if (mode < 0 || mode > 2 || layout_is_wide(lay)) return hipErrorInvalidValue;
  if (tg.kind == GM_TARGET_CUSTOM) {  // user target, runtime-compiled (gm_jit.cpp)
    HmcAdaptLaunch aa = a;
    UserTargetArg ut{tg.params, tg.D};
    void* args[] = {&aa, &ut};
    const JitKernel jk = mode == 0 ? JIT_HMC_ADAPT0 : mode == 1 ? JIT_HMC_ADAPT1 : JIT_HMC_ADAPT2;
    return with_events(ev, st, [&] {
      return jit_launch(jk, dt, tg, (unsigned)((a.h.C + 255) / 256), 256, 0, st, args);
    });
  }
  if (tg.kind == GM_TARGET_GLM) return launch_glm_hmc_adapt(dt, tg, lay, a, mode, st, ev);  // glm_kernels.hip
  using Fn = hipError_t (*)(const TargetDev&, const Layout&, const HmcAdaptLaunch&, hipStream_t, LaunchEvents);
  static const Fn table[2][3] = {
      {launch_hmc_adapt_f32_m0, launch_hmc_adapt_f32_m1, launch_hmc_adapt_f32_m2},
      {launch_hmc_adapt_f64_m0, launch_hmc_adapt_f64_m1, launch_hmc_adapt_f64_m2}};
  return table[dt == GM_F32 ? 0 : 1][mode](tg, lay, a, st, ev);
}

// A warm-up window's end with rn >= 5 collected positions (one thread per
// chain): the metric from the Welford state, the statistics reset, and the
// dual averaging restarted from eps_bar.
//   v = max((1 - regularize) * rm2/(rn-1) + regularize, max(jitter, 1e-10))
//   dinv = v (M^-1 is the VARIANCE: hmc_adapt_device.h), dsq = 1/sqrt(v)
//   eps = eps_bar;  mu = ln(10 eps);  h_bar = 0   (k = 0 and rn = 0 on the host)
template <class T>
__global__ void hmc_adapt_window_kernel(long long C, int D, double regularize, double jitter_cfg, long long rn,
                                        T* __restrict__ eps, const T* __restrict__ eps_bar,
                                        T* __restrict__ h_bar, T* __restrict__ mu, T* __restrict__ dinv,
                                        T* __restrict__ dsq, T* __restrict__ rmean, T* __restrict__ rm2) {
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const T nd = (T)(rn - 1);
  const T reg = (T)regularize;
  const T omr = (T)1 - reg;
  const T jitter = (T)(jitter_cfg > 1e-10 ? jitter_cfg : 1e-10);
  for (int i = 0; i < D; ++i) {
    const long long j = c * D + i;
    T v = omr * (rm2[j] / nd) + reg;
    v = (v >= jitter) ? v : jitter;  // a NaN variance falls back to the floor
    dinv[j] = v;
    dsq[j] = (T)1 / gsqrt(v);
    rmean[j] = (T)0;
    rm2[j] = (T)0;
  }
  const T e = eps_bar[c];
  eps[c] = e;
  mu[c] = glog((T)10 * e);
  h_bar[c] = (T)0;
}

hipError_t launch_hmc_adapt_window(gm_dtype dt, long long C, int D, double regularize, double jitter,
                                   long long rn, void* eps, const void* eps_bar, void* h_bar, void* mu,
                                   void* dinv, void* dsq, void* rmean, void* rm2, hipStream_t st) {
  const unsigned blocks = (unsigned)((C + 255) / 256);
  if (dt == GM_F32)
    hipLaunchKernelGGL(hmc_adapt_window_kernel<float>, dim3(blocks), dim3(256), 0, st, C, D, regularize, jitter,
                       rn, (float*)eps, (const float*)eps_bar, (float*)h_bar, (float*)mu, (float*)dinv,
                       (float*)dsq, (float*)rmean, (float*)rm2);
  else
    hipLaunchKernelGGL(hmc_adapt_window_kernel<double>, dim3(blocks), dim3(256), 0, st, C, D, regularize, jitter,
                       rn, (double*)eps, (const double*)eps_bar, (double*)h_bar, (double*)mu, (double*)dinv,
                       (double*)dsq, (double*)rmean, (double*)rm2);
  return hipGetLastError();
}

}  // namespace gm
