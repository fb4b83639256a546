// glm_launch.h — entry points of the GLM target's NUTS kernels
// (glm_nuts_{f32,f64}.hip, glm_nuts_rec_{f32,f64}.hip): nuts_kernel at the
// identity and the diagonal adaptive metric, recording and not.
#pragma once
#include "nuts_launch.h"

namespace gm {
#define GM_GLM_NUTS_DECL(N) \
  hipError_t N(const TargetDev& tg, const Layout& lay, NutsLaunch& a, hipStream_t st, const NutsLdsBudget& b);
GM_GLM_NUTS_DECL(launch_glm_nuts_f32)
GM_GLM_NUTS_DECL(launch_glm_nuts_f64)
GM_GLM_NUTS_DECL(launch_glm_nuts_rec_f32)
GM_GLM_NUTS_DECL(launch_glm_nuts_rec_f64)
#undef GM_GLM_NUTS_DECL

// rec: the recording instantiations, `a` is then a NutsRecLaunch
inline hipError_t launch_glm_nuts(gm_dtype dt, const TargetDev& tg, const Layout& lay, NutsLaunch& a, bool rec,
                                  hipStream_t st, const NutsLdsBudget& b) {
  if (dt == GM_F32) return rec ? launch_glm_nuts_rec_f32(tg, lay, a, st, b) : launch_glm_nuts_f32(tg, lay, a, st, b);
  return rec ? launch_glm_nuts_rec_f64(tg, lay, a, st, b) : launch_glm_nuts_f64(tg, lay, a, st, b);
}
}  // namespace gm
