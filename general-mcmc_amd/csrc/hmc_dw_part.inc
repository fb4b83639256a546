// hmc_dw_part.inc — one dtype's hmc_dw_kernel, the draw-wave form of the
// block-form HMC kernel (hmc_dw_device.h): one chain per wave at one element
// per lane, RosenbrockND, GM_DW_WAVES draw waves beside the 4 chain waves of
// a workgroup. A translation unit per dtype (hmc_dw_f32.hip and
// hmc_dw_f64.hip define GM_HMC_T) beside hmc_block_f32.hip and
// hmc_block_f64.hip.
#include "gm_internal.h"
#include "hmc_dw_device.h"

namespace gm {
hipError_t launch_hmc_dw(const RosenbrockT<GM_HMC_T>& t, const HmcLaunch& a, hipStream_t st, LaunchEvents ev) {
  static_assert(RosenbrockT<GM_HMC_T>::lf_block, "the targets of hmc_part.inc's test");
  if (a.draw_waves != GM_DW_WAVES) return hipErrorInvalidValue;
  const unsigned blocks = (unsigned)((a.C + GM_DW_CHAIN_WAVES - 1) / GM_DW_CHAIN_WAVES);
  return launch_timed(hmc_dw_kernel<GM_HMC_T, RosenbrockT<GM_HMC_T>, GM_DW_WAVES>, dim3(blocks),
                      dim3(64 * (GM_DW_CHAIN_WAVES + GM_DW_WAVES)), t.template lds_bytes<64, 1>(), st, ev, a, t);
}
}  // namespace gm
