// hmc_dw_f32.hip — hmc_dw_kernel<float, RosenbrockT<float>, GM_DW_WAVES> (hmc_dw_part.inc).
#define GM_HMC_T float
#include "hmc_dw_part.inc"
