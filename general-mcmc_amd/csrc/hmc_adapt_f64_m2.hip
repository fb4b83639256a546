// hmc_adapt_f64_m2.hip — hmc_adapt_kernel<double, ..., MODE 2> for every layout and built-in target (hmc_adapt_part.inc).
#define GM_HA_T double
#define GM_HA_MODE 2
#define GM_HA_NAME launch_hmc_adapt_f64_m2
#include "hmc_adapt_part.inc"
