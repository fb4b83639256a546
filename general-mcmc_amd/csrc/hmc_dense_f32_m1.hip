// hmc_dense_f32_m1.hip — hmc_dense_kernel<float, ..., MODE 1> for every default layout and built-in target (hmc_dense_part.inc).
#define GM_HD_T float
#define GM_HD_MODE 1
#define GM_HD_NAME launch_hmc_dense_f32_m1
#include "hmc_dense_part.inc"
