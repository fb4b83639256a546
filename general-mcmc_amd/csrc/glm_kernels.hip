// glm_kernels.hip — the GLM target's layouts, its logp_grad_kernel
// instantiations and the launcher of its hmc_adapt_kernel slices
// (glm_hmc_adapt_{f32,f64}_m{0,1,2}.hip).
#include "glm_layouts.h"
#include "util_device.h"

namespace gm {

bool glm_layout_supported(int lanes, int elems) {
#define GM_CHECK_LAYOUT(L_, E_) \
  if (lanes == L_ && elems == E_) return true;
  GM_GLM_LAYOUT_LIST(GM_CHECK_LAYOUT)
#undef GM_CHECK_LAYOUT
  return false;
}

// A whole wave per chain: the rows of the data set are split 64 ways, and a
// few thousand chains already put several waves on every SIMD.
Layout glm_default_layout(int D) {
  Layout l;
  l.lanes = 64;
  l.elems = D <= 64 ? 1 : 2;
  return l;
}

#define GM_GH_DECL(N) \
  hipError_t N(const TargetDev&, const Layout&, const HmcAdaptLaunch&, hipStream_t, LaunchEvents);
GM_GH_DECL(launch_glm_hmc_adapt_f32_m0)
GM_GH_DECL(launch_glm_hmc_adapt_f32_m1)
GM_GH_DECL(launch_glm_hmc_adapt_f32_m2)
GM_GH_DECL(launch_glm_hmc_adapt_f64_m0)
GM_GH_DECL(launch_glm_hmc_adapt_f64_m1)
GM_GH_DECL(launch_glm_hmc_adapt_f64_m2)
#undef GM_GH_DECL

hipError_t launch_glm_hmc_adapt(gm_dtype dt, const TargetDev& tg, const Layout& lay, const HmcAdaptLaunch& a, int mode,
                                hipStream_t st, LaunchEvents ev) {
  if (mode < 0 || mode > 2) return hipErrorInvalidValue;
  using Fn = hipError_t (*)(const TargetDev&, const Layout&, const HmcAdaptLaunch&, hipStream_t, LaunchEvents);
  static const Fn table[2][3] = {
      {launch_glm_hmc_adapt_f32_m0, launch_glm_hmc_adapt_f32_m1, launch_glm_hmc_adapt_f32_m2},
      {launch_glm_hmc_adapt_f64_m0, launch_glm_hmc_adapt_f64_m1, launch_glm_hmc_adapt_f64_m2}};
  return table[dt == GM_F32 ? 0 : 1][mode](tg, lay, a, st, ev);
}

template <class T>
static hipError_t glm_logp_grad_t(const TargetDev& tg, const Layout& lay, long long n, const void* x, void* logp,
                                  void* grad, hipStream_t st) {
  const GlmT<T> t = glm_target<T>(tg);
  return glm_dispatch_layout(lay, tg.D, [&]<int LPC, int E>() -> hipError_t {
    const long long threads = n * LPC;
    const unsigned blocks = (unsigned)((threads + 255) / 256);
    const size_t lds = t.template lds_bytes<LPC, E>();
    hipLaunchKernelGGL((logp_grad_kernel<T, LPC, E, GlmT<T>>), dim3(blocks), dim3(256), lds, st, n, tg.D,
                       (const T*)x, (T*)logp, (T*)grad, t);
    return hipGetLastError();
  });
}

hipError_t launch_glm_logp_grad(gm_dtype dt, const TargetDev& tg, const Layout& lay, long long n, const void* x,
                                void* logp, void* grad, hipStream_t st) {
  if (n == 0) return hipSuccess;
  return dt == GM_F32 ? glm_logp_grad_t<float>(tg, lay, n, x, logp, grad, st)
                      : glm_logp_grad_t<double>(tg, lay, n, x, logp, grad, st);
}

}  // namespace gm
