// hmc_dense_part.inc — one (dtype, MODE) slice of the hmc_dense_kernel
// instantiations, so that the four slices compile in parallel
// (hmc_dense_{f32,f64}_m{0,1}.hip define GM_HD_T, GM_HD_MODE, GM_HD_NAME).
// Built-in targets run at each dim's default layout only: E = 1,
// LPC = next_pow2(dim), 2 <= dim <= 64.
#include "gm_layouts.h"
#include "hmc_dense_device.h"

namespace gm {
hipError_t GM_HD_NAME(const TargetDev& tg, const Layout& lay, const HmcDenseLaunch& a, hipStream_t st,
                      LaunchEvents ev) {
  auto f = [&]<class T, int LPC, int E, class TG>(TG t) -> hipError_t {
    // the target's staging and the metric share the dynamic LDS; a dense
    // Gaussian target whose staged precision would push the workgroup (the
    // 3 KiB of static tables included: HMC_DENSE_LDS_DYN) past 64 KiB takes its
    // global-memory product instead (the same fma chain, the same bits):
    // f64 from dim 58 on
    if constexpr (requires { t.use_lds; }) {
      if (hmc_dense_align(t.template lds_bytes<LPC, E>()) + hmc_dense_lds<T, LPC, E>(a.h.D) > HMC_DENSE_LDS_DYN)
        t.use_lds = 0;
    }
    const size_t lds = hmc_dense_align(t.template lds_bytes<LPC, E>()) + hmc_dense_lds<T, LPC, E>(a.h.D);
    const long long threads = a.h.C * LPC;
    const unsigned blocks = (unsigned)((threads + 255) / 256);
    return launch_timed(hmc_dense_kernel<T, LPC, E, TG, GM_HD_MODE>, dim3(blocks), dim3(256), lds, st, ev, a, t);
  };
#define GM_TRY_LAYOUT(L_) \
  if (lay.lanes == L_ && lay.elems == 1) return dispatch_target<GM_HD_T, L_, 1>(tg, f);
  GM_TRY_LAYOUT(2)
  GM_TRY_LAYOUT(4)
  GM_TRY_LAYOUT(8)
  GM_TRY_LAYOUT(16)
  GM_TRY_LAYOUT(32)
  GM_TRY_LAYOUT(64)
#undef GM_TRY_LAYOUT
  return hipErrorInvalidValue;
}
}  // namespace gm
