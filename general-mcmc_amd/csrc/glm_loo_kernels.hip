// glm_loo_kernels.hip — the GLM PSIS-LOO kernels' instantiations
// (glm_loo_device.h) and their launcher.
#include "glm_loo.h"
// glm_predict_device.h defines the merge kernel as an ordinary function; its
// copy in this unit gets a name of its own, so the two objects link. That copy
// is compiled into this unit's code object and never launched (60 VGPRs, no
// LDS); GpAcc and gp_link in a header of their own would remove it.
#define glm_predict_merge glm_loo_unused_predict_merge
#include "glm_loo_device.h"
#undef glm_predict_merge
#include "glm_predict.h"

namespace gm {

long long glm_loo_max_draws() { return GL_MAX_DRAWS; }

template <class T, int KS> static hipError_t gl_product(const GlmLooLaunch& a, hipStream_t st) {
  GlmLooProdArgs<T> k;
  k.x = (const T*)a.x;
  k.off = (const T*)a.off;
  k.y = (const T*)a.y;
  k.c = (const T*)a.c;
  k.draws = (const T*)a.draws;
  k.S = a.S;
  k.stride = a.stride;
  k.M = a.M;
  k.D = a.D;
  k.family = a.family;
  k.row0 = a.row0;
  k.rows = a.rows;
  k.ll = (T*)a.ll;
  k.ld = a.ld;
  k.bad = a.bad;
  const dim3 grid((unsigned)((a.S + GP_SLAB - 1) / GP_SLAB), (unsigned)((a.rows + GP_ROWS - 1) / GP_ROWS));
  const size_t lds = (size_t)GP_STAGE * 4 * KS * sizeof(T);
  hipLaunchKernelGGL((glm_loo_product<T, KS>), grid, dim3(256), lds, st, k);
  return hipGetLastError();
}

template <class T> static hipError_t gl_launch(const GlmLooLaunch& a, hipStream_t st) {
  hipError_t e = hipMemsetAsync(a.bad, 0, (size_t)a.rows * sizeof(int), st);
  if (e != hipSuccess) return e;
  switch (glm_predict_ksteps(a.D)) {
    case 2: e = gl_product<T, 2>(a, st); break;
    case 8: e = gl_product<T, 8>(a, st); break;
    case 16: e = gl_product<T, 16>(a, st); break;
    default: e = gl_product<T, 32>(a, st); break;
  }
  if (e != hipSuccess) return e;
  GlmLooRowArgs<T> r;
  r.ll = (const T*)a.ll;
  r.ld = a.ld;
  r.S = a.S;
  r.M = a.tail_len;
  r.P = a.P;
  r.bad = a.bad;
  r.sortb = a.sortb;
  r.eb = a.eb;
  r.out = a.out;
  r.rows = a.rows;
  hipLaunchKernelGGL((glm_loo_row<T>), dim3((unsigned)a.rows), dim3(GL_THREADS), 0, st, r);
  return hipGetLastError();
}

hipError_t launch_glm_loo(gm_dtype dt, const GlmLooLaunch& a, hipStream_t st) {
  if (a.D < 1 || a.D > GLM_MAX_DIM || a.rows < 1 || a.S < 1 || a.S > GL_MAX_DRAWS || a.row0 < 0 ||
      a.row0 + a.rows > a.M || a.rows > (1LL << 20) || a.ld < a.S || (a.ld & 3) || a.tail_len < 0 ||
      a.tail_len + 1 > a.S || a.P < a.tail_len + 1 || (a.P & (a.P - 1)))
    return hipErrorInvalidValue;
  return dt == GM_F32 ? gl_launch<float>(a, st) : gl_launch<double>(a, st);
}

}  // namespace gm
