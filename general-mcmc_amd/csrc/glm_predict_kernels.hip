// glm_predict_kernels.hip — the GLM prediction kernels' instantiations
// (glm_predict_device.h) and their launcher.
#include "glm_predict.h"
#include "glm_predict_device.h"

namespace gm {

GlmPredictPlan glm_predict_plan() { return {GP_SLAB, GP_ROWS, GP_TILE}; }

int glm_predict_ksteps(int dim) { return dim <= 8 ? 2 : dim <= 32 ? 8 : dim <= 64 ? 16 : 32; }

static long long gp_slabs(long long S) { return (S + GP_SLAB - 1) / GP_SLAB; }
static long long gp_rows_pad(long long rows) { return (rows + GP_ROWS - 1) / GP_ROWS * GP_ROWS; }

size_t glm_predict_part_doubles(long long n_draws, long long rows) {
  return (size_t)gp_slabs(n_draws) * 4 * GP_FIELDS * (size_t)gp_rows_pad(rows);
}

template <class T, int KS> static hipError_t gp_main(const GlmPredictLaunch& a, hipStream_t st) {
  GlmPredictArgs<T> k;
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
  k.part = a.part;
  k.pw = (T*)a.pw;
  const dim3 grid((unsigned)gp_slabs(a.S), (unsigned)(gp_rows_pad(a.rows) / GP_ROWS));
  const size_t lds = (size_t)GP_STAGE * 4 * KS * sizeof(T);
  hipLaunchKernelGGL((glm_predict_main<T, KS>), grid, dim3(256), lds, st, k);
  return hipGetLastError();
}

template <class T> static hipError_t gp_launch(const GlmPredictLaunch& a, hipStream_t st) {
  hipError_t e;
  switch (glm_predict_ksteps(a.D)) {
    case 2: e = gp_main<T, 2>(a, st); break;
    case 8: e = gp_main<T, 8>(a, st); break;
    case 16: e = gp_main<T, 16>(a, st); break;
    default: e = gp_main<T, 32>(a, st); break;
  }
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(glm_predict_merge, dim3((unsigned)((a.rows + 255) / 256)), dim3(256), 0, st, a.part, gp_slabs(a.S),
                     gp_rows_pad(a.rows), a.row0, a.rows, a.M, a.S, a.y != nullptr ? 1 : 0, a.out);
  return hipGetLastError();
}

hipError_t launch_glm_predict(gm_dtype dt, const GlmPredictLaunch& a, hipStream_t st) {
  if (a.D < 1 || a.D > GLM_MAX_DIM || a.rows < 1 || a.S < 1 || a.row0 < 0 || a.row0 + a.rows > a.M ||
      gp_slabs(a.S) > 0x7fffffffLL || gp_rows_pad(a.rows) / GP_ROWS > 65535)
    return hipErrorInvalidValue;
  return dt == GM_F32 ? gp_launch<float>(a, st) : gp_launch<double>(a, st);
}

}  // namespace gm
