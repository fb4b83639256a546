// stats_kernels.hip — device reduction of the per-transition sampler
// statistics (gm_launch.h StatsRec, [rows][C]) over a range of record rows.
// Not in the reference.
//
// Per chain, in float64 (outputs of gm_internal.h GM_STATS_*):
//   E-BFMI = sum (E_n - E_{n-1})^2 / sum (E_n - mean E)^2, the number of
//   divergent transitions, the means of accept_stat, n_leapfrog and
//   tree_depth, and the number of transitions that reached max_depth.
// Rows whose energy is not finite are counted and left out of both energy
// sums (a difference needs both of its adjacent rows finite); every other
// quantity takes all rows.
//
//   stats_shift_kernel    each chain's shift K: its first finite energy of the
//                         range. The variance sums run on E - K, so energies
//                         near 1e4 with a spread near 1 keep their digits.
//   stats_partial_kernel  grid (chain blocks, row splits): a thread is one
//                         chain, consecutive lanes read consecutive records of
//                         one row (coalesced); partial sums [split][field][C]
//   stats_final_kernel    the splits' partials in ascending order, per chain
//   stats_total_kernel    one workgroup: the chains' sums in a fixed order
// No atomics: the result does not depend on block scheduling.
#include <hip/hip_runtime.h>

#include "gm_internal.h"

namespace gm {
namespace {

// partial sums of one (split, chain)
enum { P_N = 0, P_D1, P_D2, P_DIFF, P_DIV, P_ACC, P_NLF, P_DEPTH, P_MAXD, P_SKIP, P_COUNT };
// the chains' combined sums, kept for the totals: [S_COUNT][C]
enum { S_N = 0, S_VAR, S_DIFF, S_DIV, S_ACC, S_NLF, S_DEPTH, S_MAXD, S_SKIP, S_COUNT };

__device__ __forceinline__ bool finite_d(double v) { return v - v == 0.0; }

template <class T>
__global__ __launch_bounds__(256) void stats_shift_kernel(const StatsRec<T>* __restrict__ rec, long long C,
                                                          long long r0, long long r1, double* __restrict__ shift) {
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double k = 0.0;
  for (long long r = r0; r < r1; ++r) {
    const double e = (double)rec[r * C + c].energy;
    if (finite_d(e)) {
      k = e;
      break;
    }
  }
  shift[c] = k;
}

template <class T>
__global__ __launch_bounds__(256) void stats_partial_kernel(const StatsRec<T>* __restrict__ rec, long long C,
                                                            long long r0, long long r1, long long rows_per_split,
                                                            int max_depth, const double* __restrict__ shift,
                                                            double* __restrict__ part) {
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const long long a = r0 + (long long)blockIdx.y * rows_per_split;
  const long long b = a + rows_per_split < r1 ? a + rows_per_split : r1;
  const double k = shift[c];
  double s[P_COUNT];
#pragma unroll
  for (int f = 0; f < P_COUNT; ++f) s[f] = 0.0;
  // the row before the split, for the split's first difference
  double prev = (a > r0 && a < r1) ? (double)rec[(a - 1) * C + c].energy : __builtin_nan("");
  for (long long r = a; r < b; ++r) {
    const StatsRec<T> v = rec[r * C + c];
    const double e = (double)v.energy;
    const uint32_t w = (uint32_t)v.word;
    if (finite_d(e)) {
      const double d = e - k;
      s[P_N] += 1.0;
      s[P_D1] += d;
      s[P_D2] += d * d;
      if (finite_d(prev)) s[P_DIFF] += (e - prev) * (e - prev);
    } else {
      s[P_SKIP] += 1.0;
    }
    prev = e;
    const int depth = (int)((w >> 24) & 63u);
    s[P_DIV] += (double)((w >> 30) & 1u);
    s[P_ACC] += (double)v.accept_stat;
    s[P_NLF] += (double)(w & GM_STATS_NLF_MAX);
    s[P_DEPTH] += (double)depth;
    s[P_MAXD] += (max_depth > 0 && depth >= max_depth) ? 1.0 : 0.0;
  }
  double* o = part + (long long)blockIdx.y * P_COUNT * C + c;
#pragma unroll
  for (int f = 0; f < P_COUNT; ++f) o[f * C] = s[f];
}

__global__ __launch_bounds__(256) void stats_final_kernel(const double* __restrict__ part, long long C, int splits,
                                                          long long rows, double* __restrict__ sums,
                                                          double* __restrict__ out) {
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double s[P_COUNT];
#pragma unroll
  for (int f = 0; f < P_COUNT; ++f) s[f] = 0.0;
  for (int k = 0; k < splits; ++k)
#pragma unroll
    for (int f = 0; f < P_COUNT; ++f) s[f] += part[((long long)k * P_COUNT + f) * C + c];
  // sum (E - mean)^2 from the shifted sums
  const double var = s[P_N] > 0.0 ? s[P_D2] - s[P_D1] * s[P_D1] / s[P_N] : 0.0;
  const double n = (double)rows;
  out[GM_STATS_EBFMI * C + c] = s[P_DIFF] / var;
  out[GM_STATS_N_DIVERGENT * C + c] = s[P_DIV];
  out[GM_STATS_MEAN_ACCEPT * C + c] = s[P_ACC] / n;
  out[GM_STATS_MEAN_LEAPFROG * C + c] = s[P_NLF] / n;
  out[GM_STATS_MEAN_DEPTH * C + c] = s[P_DEPTH] / n;
  out[GM_STATS_N_MAX_DEPTH * C + c] = s[P_MAXD];
  out[GM_STATS_N_ENERGY * C + c] = s[P_N];
  out[GM_STATS_N_SKIPPED * C + c] = s[P_SKIP];
  sums[S_N * C + c] = s[P_N];
  sums[S_VAR * C + c] = var;
  sums[S_DIFF * C + c] = s[P_DIFF];
  sums[S_DIV * C + c] = s[P_DIV];
  sums[S_ACC * C + c] = s[P_ACC];
  sums[S_NLF * C + c] = s[P_NLF];
  sums[S_DEPTH * C + c] = s[P_DEPTH];
  sums[S_MAXD * C + c] = s[P_MAXD];
  sums[S_SKIP * C + c] = s[P_SKIP];
}

// thread t sums chains t, t + 256, ... in order; then a tree over the threads
__global__ __launch_bounds__(256) void stats_total_kernel(const double* __restrict__ sums, long long C,
                                                          long long rows, double* __restrict__ tot) {
  __shared__ double red[S_COUNT][256];
  const int t = threadIdx.x;
  double s[S_COUNT];
#pragma unroll
  for (int f = 0; f < S_COUNT; ++f) s[f] = 0.0;
  for (long long c = t; c < C; c += 256)
#pragma unroll
    for (int f = 0; f < S_COUNT; ++f) s[f] += sums[f * C + c];
#pragma unroll
  for (int f = 0; f < S_COUNT; ++f) red[f][t] = s[f];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w)
#pragma unroll
      for (int f = 0; f < S_COUNT; ++f) red[f][t] += red[f][t + w];
    __syncthreads();
  }
  if (t == 0) {
    const double n = (double)rows * (double)C;
    // pooled: the chains' difference sums over their sums about their own means
    tot[GM_STATS_EBFMI] = red[S_DIFF][0] / red[S_VAR][0];
    tot[GM_STATS_N_DIVERGENT] = red[S_DIV][0];
    tot[GM_STATS_MEAN_ACCEPT] = red[S_ACC][0] / n;
    tot[GM_STATS_MEAN_LEAPFROG] = red[S_NLF][0] / n;
    tot[GM_STATS_MEAN_DEPTH] = red[S_DEPTH][0] / n;
    tot[GM_STATS_N_MAX_DEPTH] = red[S_MAXD][0];
    tot[GM_STATS_N_ENERGY] = red[S_N][0];
    tot[GM_STATS_N_SKIPPED] = red[S_SKIP][0];
  }
}

}  // namespace

int stats_reduce_splits(long long C, long long rows) {
  // rows over blocks when the chains alone cannot fill the device: about 2048
  // workgroups, at least 16 rows each
  const long long cb = (C + 255) / 256;
  long long sp = (rows + 15) / 16;
  const long long cap = 2048 / cb > 1 ? 2048 / cb : 1;
  if (sp > cap) sp = cap;
  return (int)(sp < 1 ? 1 : sp);
}

size_t stats_reduce_scratch_bytes(long long C, long long rows) {
  return sizeof(double) * (size_t)C * (1 + S_COUNT + (size_t)stats_reduce_splits(C, rows) * P_COUNT);
}

hipError_t launch_stats_reduce(gm_dtype dt, const void* rec, long long C, long long r0, long long rows,
                               int max_depth, double* scratch, double* out, double* tot, hipStream_t st) {
  const int splits = stats_reduce_splits(C, rows);
  const long long rps = (rows + splits - 1) / splits;
  double* shift = scratch;
  double* sums = shift + C;
  double* part = sums + (size_t)S_COUNT * C;
  const unsigned cb = (unsigned)((C + 255) / 256);
  if (dt == GM_F32) {
    hipLaunchKernelGGL(stats_shift_kernel<float>, dim3(cb), dim3(256), 0, st, (const StatsRec<float>*)rec, C, r0,
                       r0 + rows, shift);
    hipLaunchKernelGGL(stats_partial_kernel<float>, dim3(cb, (unsigned)splits), dim3(256), 0, st,
                       (const StatsRec<float>*)rec, C, r0, r0 + rows, rps, max_depth, shift, part);
  } else {
    hipLaunchKernelGGL(stats_shift_kernel<double>, dim3(cb), dim3(256), 0, st, (const StatsRec<double>*)rec, C, r0,
                       r0 + rows, shift);
    hipLaunchKernelGGL(stats_partial_kernel<double>, dim3(cb, (unsigned)splits), dim3(256), 0, st,
                       (const StatsRec<double>*)rec, C, r0, r0 + rows, rps, max_depth, shift, part);
  }
  hipLaunchKernelGGL(stats_final_kernel, dim3(cb), dim3(256), 0, st, part, C, splits, rows, sums, out);
  hipLaunchKernelGGL(stats_total_kernel, dim3(1), dim3(256), 0, st, sums, C, rows, tot);
  return hipGetLastError();
}

}  // namespace gm
