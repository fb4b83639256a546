// glm_hmc_adapt_part.inc — one (dtype, MODE) slice of the GLM target's
// hmc_adapt_kernel instantiations, so that the six slices compile in parallel
// (glm_hmc_adapt_{f32,f64}_m{0,1,2}.hip define GM_GH_T, GM_GH_MODE, GM_GH_NAME).
#include "glm_layouts.h"
#include "hmc_adapt_device.h"

namespace gm {
hipError_t GM_GH_NAME(const TargetDev& tg, const Layout& lay, const HmcAdaptLaunch& a, hipStream_t st,
                      LaunchEvents ev) {
  using T = GM_GH_T;
  const GlmT<T> t = glm_target<T>(tg);
  return glm_dispatch_layout(lay, tg.D, [&]<int LPC, int E>() -> hipError_t {
    const size_t lds = t.template lds_bytes<LPC, E>();
    const long long threads = a.h.C * LPC;
    const unsigned blocks = (unsigned)((threads + 255) / 256);
    return launch_timed(hmc_adapt_kernel<T, LPC, E, GlmT<T>, GM_GH_MODE>, dim3(blocks), dim3(256), lds, st, ev, a, t);
  });
}
}  // namespace gm
