// hmc_block_f32.hip — hmc_kernel<float, 64, 1, RosenbrockT<float>, GM_LF_BLOCK> (hmc_block_part.inc).
#define GM_HMC_T float
#include "hmc_block_part.inc"
