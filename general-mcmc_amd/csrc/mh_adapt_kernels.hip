// mh_adapt_kernels.hip — launchers of mh_adapt_kernel (mh_adapt_device.h:
// MH with a per-chain proposal scale and a per-chain diagonal shape, and their
// warm-up) and the window-end update that runs between two of its launches.
// The kernel's instantiations are in mh_adapt_{f32,f64}_m{0,1,2}.hip.
#include "gm_jit.h"
#include "gm_rng.h"

namespace gm {

#define GM_MA_DECL(N) \
  hipError_t N(const TargetDev&, const Layout&, const MhAdaptLaunch&, hipStream_t, LaunchEvents);
GM_MA_DECL(launch_mh_adapt_f32_m0)
GM_MA_DECL(launch_mh_adapt_f32_m1)
GM_MA_DECL(launch_mh_adapt_f32_m2)
GM_MA_DECL(launch_mh_adapt_f64_m0)
GM_MA_DECL(launch_mh_adapt_f64_m1)
GM_MA_DECL(launch_mh_adapt_f64_m2)
#undef GM_MA_DECL

hipError_t launch_mh_adapt(gm_dtype dt, const TargetDev& tg, const Layout& lay, const MhAdaptLaunch& a, int mode,
                           hipStream_t st, LaunchEvents ev) {
  if (mode < 0 || mode > 2 || layout_is_wide(lay)) return hipErrorInvalidValue;
  if (tg.kind == GM_TARGET_CUSTOM) {  // user target, runtime-compiled (gm_jit.cpp)
    MhAdaptLaunch aa = a;
    UserTargetArg ut{tg.params, tg.D};
    void* args[] = {&aa, &ut};
    const JitKernel jk = mode == 0 ? JIT_MH_ADAPT0 : mode == 1 ? JIT_MH_ADAPT1 : JIT_MH_ADAPT2;
    return with_events(ev, st, [&] {
      return jit_launch(jk, dt, tg, (unsigned)((a.m.C + 255) / 256), 256, 0, st, args);
    });
  }
  using Fn = hipError_t (*)(const TargetDev&, const Layout&, const MhAdaptLaunch&, hipStream_t, LaunchEvents);
  static const Fn table[2][3] = {
      {launch_mh_adapt_f32_m0, launch_mh_adapt_f32_m1, launch_mh_adapt_f32_m2},
      {launch_mh_adapt_f64_m0, launch_mh_adapt_f64_m1, launch_mh_adapt_f64_m2}};
  return table[dt == GM_F32 ? 0 : 1][mode](tg, lay, a, st, ev);
}

// A warm-up window's end with rn >= 5 collected positions (one thread per
// chain): the proposal shape from the Welford state, the statistics reset, and
// the dual averaging restarted from scale_bar.
//   v = max((1 - regularize) * rm2/(rn-1) + regularize, max(jitter, 1e-10))
//   diag = sqrt(v)   (a standard deviation: mh_adapt_device.h)
//   scale = scale_bar;  mu = ln(10 scale);  h_bar = 0   (k = 0 and rn = 0 on the host)
template <class T>
__global__ void mh_adapt_window_kernel(long long C, int D, double regularize, double jitter_cfg, long long rn,
                                       T* __restrict__ scale, const T* __restrict__ scale_bar,
                                       T* __restrict__ h_bar, T* __restrict__ mu, T* __restrict__ diag,
                                       T* __restrict__ rmean, T* __restrict__ rm2) {
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
    diag[j] = gsqrt(v);
    rmean[j] = (T)0;
    rm2[j] = (T)0;
  }
  const T e = scale_bar[c];
  scale[c] = e;
  mu[c] = glog((T)10 * e);
  h_bar[c] = (T)0;
}

hipError_t launch_mh_adapt_window(gm_dtype dt, long long C, int D, double regularize, double jitter, long long rn,
                                  void* scale, const void* scale_bar, void* h_bar, void* mu, void* diag,
                                  void* rmean, void* rm2, hipStream_t st) {
  const unsigned blocks = (unsigned)((C + 255) / 256);
  if (dt == GM_F32)
    hipLaunchKernelGGL(mh_adapt_window_kernel<float>, dim3(blocks), dim3(256), 0, st, C, D, regularize, jitter, rn,
                       (float*)scale, (const float*)scale_bar, (float*)h_bar, (float*)mu, (float*)diag,
                       (float*)rmean, (float*)rm2);
  else
    hipLaunchKernelGGL(mh_adapt_window_kernel<double>, dim3(blocks), dim3(256), 0, st, C, D, regularize, jitter, rn,
                       (double*)scale, (const double*)scale_bar, (double*)h_bar, (double*)mu, (double*)diag,
                       (double*)rmean, (double*)rm2);
  return hipGetLastError();
}

}  // namespace gm
