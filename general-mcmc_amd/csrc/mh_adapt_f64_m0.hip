// mh_adapt_f64_m0.hip — mh_adapt_kernel<double, ..., MODE 0> for every layout and built-in target (mh_adapt_part.inc).
#define GM_MA_T double
#define GM_MA_MODE 0
#define GM_MA_NAME launch_mh_adapt_f64_m0
#include "mh_adapt_part.inc"
