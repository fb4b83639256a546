// hmc_block_part.inc — one dtype's hmc_kernel with the block leapfrog loop
// form (GM_LF_BLOCK, hmc_device.h): one chain per wave at one element per lane,
// RosenbrockND. A translation unit per dtype beside hmc_f32.hip and
// hmc_f64.hip (hmc_block_f32.hip and hmc_block_f64.hip define GM_HMC_T), so
// that the long straight-line block compiles in parallel with them.
#include "gm_internal.h"
#include "hmc_device.h"

namespace gm {
hipError_t launch_hmc_block(const RosenbrockT<GM_HMC_T>& t, const HmcLaunch& a, hipStream_t st, LaunchEvents ev) {
  static_assert(RosenbrockT<GM_HMC_T>::lf_block, "the targets of hmc_part.inc's test");
  const unsigned blocks = (unsigned)((a.C * 64 + 255) / 256);
  return launch_timed(hmc_kernel<GM_HMC_T, 64, 1, RosenbrockT<GM_HMC_T>, GM_LF_BLOCK>, dim3(blocks), dim3(256),
                      t.template lds_bytes<64, 1>(), st, ev, a, t);
}
}  // namespace gm
