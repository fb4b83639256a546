// glm_hmc_adapt_f32_m2.hip — hmc_adapt_kernel<float, ..., GlmT, MODE 2> for every GLM layout (glm_hmc_adapt_part.inc).
#define GM_GH_T float
#define GM_GH_MODE 2
#define GM_GH_NAME launch_glm_hmc_adapt_f32_m2
#include "glm_hmc_adapt_part.inc"
