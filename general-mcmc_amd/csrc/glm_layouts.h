// glm_layouts.h — the layouts compiled for the GLM target (glm_device.h) and
// the device-side target from the host's view. The target has a layout list
// of its own, outside gm_layouts.h's dispatch: a chain's lanes split the rows
// of the data set, so the list is chosen for that (whole waves or quarter
// waves, LPC * E a multiple of GLM_CH), and the other targets' translation
// units compile what they always did.
#pragma once
#include "glm_device.h"
#include "gm_internal.h"

// X(LPC, E): 16 x 2 (dim <= 32, four chains per wave: for many chains),
// 64 x 1 (dim <= 64), 64 x 2 (dim <= 128)
#define GM_GLM_LAYOUT_LIST(X) \
  X(16, 2)                    \
  X(64, 1)                    \
  X(64, 2)

namespace gm {

template <class T> inline GlmT<T> glm_target(const TargetDev& tg) {
  GlmT<T> t;
  const T* base = (const T*)tg.glm;
  t.iv = base;
  t.y = base + tg.glm_dp;
  t.off = t.y + tg.glm_np;
  t.xt = t.off + tg.glm_np;
  t.N = tg.glm_n;
  t.Np = tg.glm_np;
  t.D = tg.D;
  t.Dp = tg.glm_dp;
  t.family = tg.glm_family;
  return t;
}

// f.template operator()<LPC, E>() for the runtime layout
template <class F> hipError_t glm_dispatch_layout(const Layout& lay, int D, F&& f) {
  if ((long long)lay.lanes * lay.elems < D) return hipErrorInvalidValue;
#define GM_TRY_LAYOUT(L_, E_) \
  if (lay.lanes == L_ && lay.elems == E_) return f.template operator()<L_, E_>();
  GM_GLM_LAYOUT_LIST(GM_TRY_LAYOUT)
#undef GM_TRY_LAYOUT
  return hipErrorInvalidValue;
}

}  // namespace gm
