// hmc_dw_f64.hip — hmc_dw_kernel<double, RosenbrockT<double>, GM_DW_WAVES> (hmc_dw_part.inc).
#define GM_HMC_T double
#include "hmc_dw_part.inc"
