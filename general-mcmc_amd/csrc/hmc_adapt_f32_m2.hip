// hmc_adapt_f32_m2.hip — hmc_adapt_kernel<float, ..., MODE 2> for every layout and built-in target (hmc_adapt_part.inc).
#define GM_HA_T float
#define GM_HA_MODE 2
#define GM_HA_NAME launch_hmc_adapt_f32_m2
#include "hmc_adapt_part.inc"
