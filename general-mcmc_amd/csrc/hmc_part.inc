// hmc_part.inc — one dtype's slice of the hmc_kernel instantiations (every
// layout and built-in target), so that the two slices compile in parallel
// (hmc_f32.hip and hmc_f64.hip define GM_HMC_T and GM_HMC_NAME).
#include "gm_layouts.h"
#include "hmc_device.h"

namespace gm {
// hmc_kernel<T, 64, 1, RosenbrockT<T>, GM_LF_BLOCK> (hmc_block_f32.hip, hmc_block_f64.hip)
hipError_t launch_hmc_block(const RosenbrockT<GM_HMC_T>& t, const HmcLaunch& a, hipStream_t st, LaunchEvents ev);
// hmc_dw_kernel<T, RosenbrockT<T>, GM_DW_WAVES> (hmc_dw_f32.hip, hmc_dw_f64.hip)
hipError_t launch_hmc_dw(const RosenbrockT<GM_HMC_T>& t, const HmcLaunch& a, hipStream_t st, LaunchEvents ev);

hipError_t GM_HMC_NAME(const TargetDev& tg, const Layout& lay, const HmcLaunch& a, hipStream_t st,
                       LaunchEvents ev) {
  // (two chains per wave on packed f32 arithmetic, 13 VALU per two
  // chain-leapfrogs instead of 22, bitwise equal, measured no faster: at the
  // 2 waves per SIMD it leaves at 4096 chains the loop is latency-bound,
  // profiles/r04/ab_hmc_packed_and_fma_order.log; not kept)
  auto f = [&]<class T, int LPC, int E, class TG>(TG t) -> hipError_t {
    const size_t lds = t.template lds_bytes<LPC, E>();
    const long long threads = a.C * LPC;
    const unsigned blocks = (unsigned)((threads + 255) / 256);
    // one chain per wave with 1 or 2 elements per lane (the many-chain
    // shapes): the leapfrog loop form is compiled in, so each of the S
    // unrolled block positions carries one form instead of three
    if constexpr (LPC == 64 && E <= 2) {
      // the block form: one element per lane and the targets with
      // lf_block, in a unit of its own (hmc_block_part.inc); elsewhere the
      // number runs the long form
      if constexpr (E == 1 && requires { TG::lf_block; }) {
        // ... and its draw-wave form (hmc_dw_part.inc) where the launch asks for it
        if (a.lf_unroll == GM_LF_BLOCK && a.draw_waves == GM_DW_WAVES) return launch_hmc_dw(t, a, st, ev);
        if (a.lf_unroll == GM_LF_BLOCK) return launch_hmc_block(t, a, st, ev);
      }
      if (a.lf_unroll == GM_LF_LONG || a.lf_unroll == GM_LF_BLOCK)
        return launch_timed(hmc_kernel<T, LPC, E, TG, GM_LF_LONG>, dim3(blocks), dim3(256), lds, st, ev, a, t);
      if (a.lf_unroll == 4)
        return launch_timed(hmc_kernel<T, LPC, E, TG, 4>, dim3(blocks), dim3(256), lds, st, ev, a, t);
      if (a.lf_unroll == 2)
        return launch_timed(hmc_kernel<T, LPC, E, TG, 2>, dim3(blocks), dim3(256), lds, st, ev, a, t);
      return launch_timed(hmc_kernel<T, LPC, E, TG, 1>, dim3(blocks), dim3(256), lds, st, ev, a, t);
    } else {
      return launch_timed(hmc_kernel<T, LPC, E, TG>, dim3(blocks), dim3(256), lds, st, ev, a, t);
    }
  };
#define GM_TRY_LAYOUT(L_, E_) \
  if (lay.lanes == L_ && lay.elems == E_) return dispatch_target<GM_HMC_T, L_, E_>(tg, f);
  GM_LAYOUT_LIST(GM_TRY_LAYOUT)
#undef GM_TRY_LAYOUT
  return hipErrorInvalidValue;
}
}  // namespace gm
