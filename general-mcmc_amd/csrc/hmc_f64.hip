// hmc_f64.hip — hmc_kernel<double, ...> for every layout and built-in target (hmc_part.inc).
#define GM_HMC_T double
#define GM_HMC_NAME launch_hmc_f64
#include "hmc_part.inc"
