// mh_adapt_f32_m2.hip — mh_adapt_kernel<float, ..., MODE 2> for every layout and built-in target (mh_adapt_part.inc).
#define GM_MA_T float
#define GM_MA_MODE 2
#define GM_MA_NAME launch_mh_adapt_f32_m2
#include "mh_adapt_part.inc"
