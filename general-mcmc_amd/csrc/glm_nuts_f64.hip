// glm_nuts_f64.hip — nuts_kernel<double, ..., GlmT> for every GLM layout, identity and diagonal metric (glm_nuts_part.inc).
#define GM_GN_T double
#define GM_GN_REC 0
#define GM_GN_NAME launch_glm_nuts_f64
#include "glm_nuts_part.inc"
