// glm_hmc_adapt_f32_m0.hip — hmc_adapt_kernel<float, ..., GlmT, MODE 0> for every GLM layout (glm_hmc_adapt_part.inc).
#define GM_GH_T float
#define GM_GH_MODE 0
#define GM_GH_NAME launch_glm_hmc_adapt_f32_m0
#include "glm_hmc_adapt_part.inc"
