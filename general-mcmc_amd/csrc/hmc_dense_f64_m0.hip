// hmc_dense_f64_m0.hip — hmc_dense_kernel<double, ..., MODE 0> for every default layout and built-in target (hmc_dense_part.inc).
#define GM_HD_T double
#define GM_HD_MODE 0
#define GM_HD_NAME launch_hmc_dense_f64_m0
#include "hmc_dense_part.inc"
