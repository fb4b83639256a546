// glm_hmc_adapt_f64_m1.hip — hmc_adapt_kernel<double, ..., GlmT, MODE 1> for every GLM layout (glm_hmc_adapt_part.inc).
#define GM_GH_T double
#define GM_GH_MODE 1
#define GM_GH_NAME launch_glm_hmc_adapt_f64_m1
#include "glm_hmc_adapt_part.inc"
