// glm_nuts_part.inc — one (dtype, recording or not) slice of the GLM target's
// nuts_kernel instantiations: every GLM layout at the identity metric and the
// diagonal adaptive metric (glm_nuts*_{f32,f64}.hip define GM_GN_T, GM_GN_REC,
// GM_GN_NAME), so that the four slices compile in parallel.
#include "glm_layouts.h"
#include "nuts_device.h"
#include "glm_launch.h"

namespace gm {
hipError_t GM_GN_NAME(const TargetDev& tg, const Layout& lay, NutsLaunch& a, hipStream_t st, const NutsLdsBudget& b) {
  using T = GM_GN_T;
  constexpr bool REC = GM_GN_REC != 0;
  if (a.mass_mode != 0 && a.mass_mode != 1) return hipErrorInvalidValue;
  typename NutsLaunchOf<REC>::type& ka = static_cast<typename NutsLaunchOf<REC>::type&>(a);
  const GlmT<T> t = glm_target<T>(tg);
  return glm_dispatch_layout(lay, tg.D, [&]<int LPC, int E>() -> hipError_t {
    const long long threads = a.C * LPC;
    const unsigned blocks = (unsigned)((threads + 255) / 256);
    const size_t lds = nuts_size_lds(a, b, blocks, t.template lds_bytes<LPC, E>(), LPC, E, sizeof(T));
    if (a.mass_mode == 1)
      hipLaunchKernelGGL((nuts_kernel<T, LPC, E, GlmT<T>, 1, REC>), dim3(blocks), dim3(256), lds, st, ka, t);
    else
      hipLaunchKernelGGL((nuts_kernel<T, LPC, E, GlmT<T>, 0, REC>), dim3(blocks), dim3(256), lds, st, ka, t);
    return hipGetLastError();
  });
}
}  // namespace gm
