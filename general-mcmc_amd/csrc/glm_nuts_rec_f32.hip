// glm_nuts_rec_f32.hip — the recording nuts_kernel<float, ..., GlmT> for every GLM layout (glm_nuts_part.inc).
#define GM_GN_T float
#define GM_GN_REC 1
#define GM_GN_NAME launch_glm_nuts_rec_f32
#include "glm_nuts_part.inc"
