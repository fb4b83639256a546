// hmc_f32.hip — hmc_kernel<float, ...> for every layout and built-in target (hmc_part.inc).
#define GM_HMC_T float
#define GM_HMC_NAME launch_hmc_f32
#include "hmc_part.inc"
