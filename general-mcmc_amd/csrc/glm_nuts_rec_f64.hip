// glm_nuts_rec_f64.hip — the recording nuts_kernel<double, ..., GlmT> for every GLM layout (glm_nuts_part.inc).
#define GM_GN_T double
#define GM_GN_REC 1
#define GM_GN_NAME launch_glm_nuts_rec_f64
#include "glm_nuts_part.inc"
