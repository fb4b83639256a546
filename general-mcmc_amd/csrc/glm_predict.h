// glm_predict.h — host-side declarations of the GLM prediction kernels
// (glm_predict_kernels.hip), used by gmcmc_predict.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/gmcmc.h"

namespace gm {

// the decomposition's sizes (glm_predict_device.h)
struct GlmPredictPlan {
  int slab, rows, tile;
};
GlmPredictPlan glm_predict_plan();
// k-steps of 4 columns of the instantiation that takes dim columns (2, 8, 16 or 32)
int glm_predict_ksteps(int dim);
size_t glm_predict_part_doubles(long long n_draws, long long rows);

// One launch pair over data rows [row0, row0 + rows): the main kernel's
// partials into part, then their merge into out [7][M] (float64).
// x [M][4 ksteps] zero-padded, off / y / c [M] (y and c null together), draws
// [S] rows of stride elements, pw [S][M] or null; all device memory of dtype.
struct GlmPredictLaunch {
  const void *x, *off, *y, *c, *draws;
  long long S, stride, M;
  int D, family;
  long long row0, rows;
  double* part;
  double* out;
  void* pw;
};
hipError_t launch_glm_predict(gm_dtype dt, const GlmPredictLaunch& a, hipStream_t st);

}  // namespace gm
