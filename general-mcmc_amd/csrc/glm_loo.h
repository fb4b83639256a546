// glm_loo.h — host-side declarations of the GLM PSIS-LOO kernels
// (glm_loo_kernels.hip), used by gmcmc_loo.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/gmcmc.h"

namespace gm {

long long glm_loo_max_draws();

// One group of data rows [row0, row0 + rows): the product kernel fills
// ll [rows][ld] and bad [rows] (zeroed here), the row kernel leaves the sorted
// slots in sortb [rows][P] (slot 0 the cutoff, 1 .. M the tail ascending) and
// elpd_loo, pareto_k in out [2][rows]. x [M][4 ksteps] zero-padded, off / y /
// c [M], draws [S] rows of stride elements; all device memory, of dtype
// unless typed.
struct GlmLooLaunch {
  const void *x, *off, *y, *c, *draws;
  long long S, stride, M;
  int D, family;
  long long row0, rows;
  void* ll;
  long long ld;
  int* bad;
  long long tail_len, P;
  double *sortb, *eb, *out;
};
hipError_t launch_glm_loo(gm_dtype dt, const GlmLooLaunch& a, hipStream_t st);

}  // namespace gm
