// hmc_block_f64.hip — hmc_kernel<double, 64, 1, RosenbrockT<double>, GM_LF_BLOCK> (hmc_block_part.inc).
#define GM_HMC_T double
#include "hmc_block_part.inc"
