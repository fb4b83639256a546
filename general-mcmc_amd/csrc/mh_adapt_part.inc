// mh_adapt_part.inc — one (dtype, MODE) slice of the mh_adapt_kernel
// instantiations, so that the six slices compile in parallel
// (mh_adapt_{f32,f64}_m{0,1,2}.hip define GM_MA_T, GM_MA_MODE, GM_MA_NAME).
#include "gm_layouts.h"
#include "mh_adapt_device.h"

namespace gm {
hipError_t GM_MA_NAME(const TargetDev& tg, const Layout& lay, const MhAdaptLaunch& a, hipStream_t st,
                      LaunchEvents ev) {
  auto f = [&]<class T, int LPC, int E, class TG>(TG t) -> hipError_t {
    const size_t lds = t.template lds_bytes<LPC, E>();
    const long long threads = a.m.C * LPC;
    const unsigned blocks = (unsigned)((threads + 255) / 256);
    return launch_timed(mh_adapt_kernel<T, LPC, E, TG, GM_MA_MODE>, dim3(blocks), dim3(256), lds, st, ev, a, t);
  };
#define GM_TRY_LAYOUT(L_, E_) \
  if (lay.lanes == L_ && lay.elems == E_) return dispatch_target<GM_MA_T, L_, E_>(tg, f);
  GM_LAYOUT_LIST(GM_TRY_LAYOUT)
#undef GM_TRY_LAYOUT
  return hipErrorInvalidValue;
}
}  // namespace gm
