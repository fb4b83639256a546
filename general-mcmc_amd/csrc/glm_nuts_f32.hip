// glm_nuts_f32.hip — nuts_kernel<float, ..., GlmT> for every GLM layout, identity and diagonal metric (glm_nuts_part.inc).
#define GM_GN_T float
#define GM_GN_REC 0
#define GM_GN_NAME launch_glm_nuts_f32
#include "glm_nuts_part.inc"
