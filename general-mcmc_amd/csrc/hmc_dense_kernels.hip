// hmc_dense_kernels.hip — launchers of hmc_dense_kernel (hmc_dense_device.h:
// HMC with per-chain step sizes and one dense metric shared by all chains),
// the pooled statistics of its warm-up and the window-end update. The
// kernel's instantiations are in hmc_dense_{f32,f64}_m{0,1}.hip.
//
// Pooled statistics (all float64): a warm-up launch stores each transition's
// post-accept positions to a scratch slab [rows][C][D]; after the launch
//   hmc_dense_pivot_kernel   c0 = mean over chains of the window's first row
//   hmc_dense_gram_kernel    per row and per block of GD_CB chains, the sums
//                            of (x - c0) and of (x - c0)(x - c0)^T, the latter
//                            on the f64 matrix cores (v_mfma_f64_16x16x4_f64)
//   hmc_dense_gram_reduce_kernel  per row, the blocks' partials added in block
//                            order; the rows added to s1 and S2 in row order
// The partition over chains depends on C only and the rows are added one
// after another, so the sums do not depend on how the run was cut into
// launches. No floating-point atomics.
#include <algorithm>

#include "gm_jit.h"
#include "gm_plan.h"
#include "gm_rng.h"

namespace gm {

#define GM_HD_DECL(N) \
  hipError_t N(const TargetDev&, const Layout&, const HmcDenseLaunch&, hipStream_t, LaunchEvents);
GM_HD_DECL(launch_hmc_dense_f32_m0)
GM_HD_DECL(launch_hmc_dense_f32_m1)
GM_HD_DECL(launch_hmc_dense_f64_m0)
GM_HD_DECL(launch_hmc_dense_f64_m1)
#undef GM_HD_DECL

hipError_t launch_hmc_dense(gm_dtype dt, const TargetDev& tg, const Layout& lay, const HmcDenseLaunch& a,
                            int mode, hipStream_t st, LaunchEvents ev) {
  if (mode < 0 || mode > 1) return hipErrorInvalidValue;
  if (tg.kind == GM_TARGET_CUSTOM) {  // user target, runtime-compiled (gm_jit.cpp) at layout (1, dim)
    if (lay.lanes != 1 || lay.elems != a.h.D || a.h.D > GM_DENSE_MAX_DIM) return hipErrorInvalidValue;
    HmcDenseLaunch aa = a;
    UserTargetArg ut{tg.params, tg.D};
    void* args[] = {&aa, &ut};
    const size_t esz = dt == GM_F32 ? 4 : 8;
    const unsigned block = hmc_dense_user_block(a.h.D, esz);
    const size_t lds = hmc_dense_lds_user(a.h.D, (int)block, esz);
    return with_events(ev, st, [&] {
      return jit_launch(mode == 0 ? JIT_HMC_DENSE0 : JIT_HMC_DENSE1, dt, tg,
                        (unsigned)((a.h.C + block - 1) / block), block, lds, st, args);
    });
  }
  if (lay.elems != 1 || lay.lanes > 64) return hipErrorInvalidValue;
  using Fn = hipError_t (*)(const TargetDev&, const Layout&, const HmcDenseLaunch&, hipStream_t, LaunchEvents);
  static const Fn table[2][2] = {{launch_hmc_dense_f32_m0, launch_hmc_dense_f32_m1},
                                 {launch_hmc_dense_f64_m0, launch_hmc_dense_f64_m1}};
  return table[dt == GM_F32 ? 0 : 1][mode](tg, lay, a, st, ev);
}

// ---- pooled statistics ------------------------------------------------------
constexpr int GD_CB = 1024;           // chains per gram block (256 per wave)
constexpr int GD_PE = 64 * 64 + 64;   // doubles of one partial: Gram [64][64], row sums [64]

// c0[i] = mean over chains of x[c][i] (one block; thread (part, i) sums the
// chains c = part mod 4 in ascending order, the four parts are added in order)
template <class T>
__global__ __launch_bounds__(256) void hmc_dense_pivot_kernel(const T* __restrict__ x, long long C, int D,
                                                              double* __restrict__ c0) {
  __shared__ double ps[4][64];
  const int i = threadIdx.x & 63, part = threadIdx.x >> 6;
  double s = 0.0;
  if (i < D)
    for (long long c = part; c < C; c += 4) s += (double)x[c * D + i];
  ps[part][i] = s;
  __syncthreads();
  if (part == 0 && i < D) c0[i] = (((ps[0][i] + ps[1][i]) + ps[2][i]) + ps[3][i]) / (double)C;
}

using f64x4 = __attribute__((ext_vector_type(4))) double;

// grid (blocks of GD_CB chains, rows). A wave owns 256 chains of the row and
// accumulates the upper-triangle 16x16 tiles of their Gram matrix with
// v_mfma_f64_16x16x4_f64 (K = 4 chains per instruction; A = B = the same
// fragment, lane l holding y_{chain k = l/16}[i = 16 tb + l%16], y = x - c0);
// the four waves' tiles are then added in wave order through LDS.
template <class T>
__global__ __launch_bounds__(256) void hmc_dense_gram_kernel(const T* __restrict__ x, long long C, int D,
                                                             const double* __restrict__ c0,
                                                             double* __restrict__ part) {
  __shared__ double G[64 * 64];
  __shared__ double R[4][4][64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int kk = lane >> 4, ii = lane & 15;
  const long long t = blockIdx.y;
  const T* __restrict__ xr = x + t * C * D;
  double cz[4], rs[4];
  f64x4 acc[10];
#pragma unroll
  for (int tb = 0; tb < 4; ++tb) {
    const int i = 16 * tb + ii;
    cz[tb] = (i < D) ? c0[i] : 0.0;
    rs[tb] = 0.0;
  }
#pragma unroll
  for (int i = 0; i < 10; ++i) acc[i] = (f64x4){0.0, 0.0, 0.0, 0.0};
  const long long cbase = (long long)blockIdx.x * GD_CB + wave * 256;
  for (int ks = 0; ks < 64; ++ks) {
    if (cbase + 4 * ks >= C) break;  // wave-uniform
    const long long c = cbase + 4 * ks + kk;
    double f[4];
#pragma unroll
    for (int tb = 0; tb < 4; ++tb) {
      const int i = 16 * tb + ii;
      f[tb] = (c < C && i < D) ? (double)xr[c * D + i] - cz[tb] : 0.0;
      rs[tb] += f[tb];
    }
    int ti = 0;
#pragma unroll
    for (int tb = 0; tb < 4; ++tb)
#pragma unroll
      for (int tb2 = tb; tb2 < 4; ++tb2, ++ti)
        if (tb2 * 16 < D) acc[ti] = __builtin_amdgcn_mfma_f64_16x16x4f64(f[tb], f[tb2], acc[ti], 0, 0, 0);
  }
#pragma unroll
  for (int tb = 0; tb < 4; ++tb) R[wave][kk][16 * tb + ii] = rs[tb];
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
      int ti = 0;
#pragma unroll
      for (int tb = 0; tb < 4; ++tb)
#pragma unroll
        for (int tb2 = tb; tb2 < 4; ++tb2, ++ti) {
          // C/D map of the f64 MFMA: col = lane%16, row = lane/16 + 4*r
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int idx = (16 * tb + kk + 4 * r) * 64 + 16 * tb2 + ii;
            G[idx] = (w == 0) ? acc[ti][r] : G[idx] + acc[ti][r];
          }
        }
    }
    __syncthreads();
  }
  double* __restrict__ o = part + (t * gridDim.x + blockIdx.x) * GD_PE;
  for (int idx = tid; idx < 64 * 64; idx += 256) {
    const int row = idx >> 6, col = idx & 63;
    o[idx] = ((row >> 4) <= (col >> 4) && row < D && col < D) ? G[idx] : 0.0;
  }
  if (tid < 64) {
    double s = 0.0;
    for (int w = 0; w < 4; ++w)
      for (int k = 0; k < 4; ++k) s += R[w][k][tid];
    o[64 * 64 + tid] = s;
  }
}

// one thread per entry of S2 (D*D) and s1 (D): per row the blocks' partials in
// block order, the rows in row order
__global__ void hmc_dense_gram_reduce_kernel(const double* __restrict__ part, int rows, int nb, int D,
                                             double* __restrict__ s1, double* __restrict__ S2) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= D * D + D) return;
  int src;
  double* dst;
  if (idx < D * D) {
    const int i = idx / D, j = idx - i * D;
    src = ((i >> 4) <= (j >> 4)) ? i * 64 + j : j * 64 + i;
    dst = S2 + idx;
  } else {
    src = 64 * 64 + (idx - D * D);
    dst = s1 + (idx - D * D);
  }
  double a = *dst;
  for (int t = 0; t < rows; ++t) {
    const double* p = part + (long long)t * nb * GD_PE + src;
    double g = p[0];
    for (int b = 1; b < nb; ++b) g += p[(long long)b * GD_PE];
    a += g;
  }
  *dst = a;
}

static int hmc_dense_gram_blocks(long long C) { return (int)((C + GD_CB - 1) / GD_CB); }
static size_t hmc_dense_gram_part_bytes(long long C, int rows) {
  return (size_t)rows * hmc_dense_gram_blocks(C) * GD_PE * sizeof(double);
}

static hipError_t launch_hmc_dense_pivot(gm_dtype dt, const void* x, long long C, int D, double* c0,
                                         hipStream_t st) {
  if (dt == GM_F32) hipLaunchKernelGGL(hmc_dense_pivot_kernel<float>, dim3(1), dim3(256), 0, st, (const float*)x, C, D, c0);
  else hipLaunchKernelGGL(hmc_dense_pivot_kernel<double>, dim3(1), dim3(256), 0, st, (const double*)x, C, D, c0);
  return hipGetLastError();
}

// adds rows [0, rows) of x [rows][C][D] into s1 and S2; part holds
// hmc_dense_gram_part_bytes(C, rows) bytes
static hipError_t launch_hmc_dense_gram(gm_dtype dt, const void* x, int rows, long long C, int D, const double* c0,
                                        double* part, double* s1, double* S2, hipStream_t st) {
  const int nb = hmc_dense_gram_blocks(C);
  const dim3 grid((unsigned)nb, (unsigned)rows);
  if (dt == GM_F32)
    hipLaunchKernelGGL(hmc_dense_gram_kernel<float>, grid, dim3(256), 0, st, (const float*)x, C, D, c0, part);
  else
    hipLaunchKernelGGL(hmc_dense_gram_kernel<double>, grid, dim3(256), 0, st, (const double*)x, C, D, c0, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int n = D * D + D;
  hipLaunchKernelGGL(hmc_dense_gram_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, st, (const double*)part,
                     rows, nb, D, s1, S2);
  return hipGetLastError();
}

int pooled_scratch_ensure(PooledScratch& ps, long long rows, long long C, int D, size_t esz) {
  const long long rb = gram_rows_for(hmc_dense_gram_part_bytes(C, 1));
  int rc = ensure_buf(&ps.slab, &ps.slab_bytes, (size_t)rows * (size_t)C * D * esz);
  if (!rc) rc = ensure_buf(&ps.part, &ps.part_bytes, hmc_dense_gram_part_bytes(C, (int)std::min(rb, rows)));
  return rc;
}

hipError_t pooled_accumulate(gm_dtype dt, const PooledScratch& ps, long long used, long long C, int D,
                             long long* rn, double* c0, double* s1, double* S2, hipStream_t st) {
  const size_t row_bytes = (size_t)C * D * (dt == GM_F32 ? 4 : 8);
  const long long rb = gram_rows_for(hmc_dense_gram_part_bytes(C, 1));
  hipError_t e = hipSuccess;
  if (*rn == 0) e = launch_hmc_dense_pivot(dt, ps.slab, C, D, c0, st);
  for (long long r = 0; r < used && e == hipSuccess; r += rb) {
    const int rows = (int)std::min(rb, used - r);
    e = launch_hmc_dense_gram(dt, (const char*)ps.slab + (size_t)r * row_bytes, rows, C, D, c0, (double*)ps.part, s1,
                              S2, st);
  }
  *rn += used;
  return e;
}

// ---- window end / metric set --------------------------------------------------
// One workgroup. from_stats: Sigma = (1 - reg) S + reg I with the diagonal
// floored at max(jitter, 1e-10), S = (S2 - s1 s1^T / n) / (n - 1); otherwise
// Sigma = sig_in. Then the Cholesky factorisation Sigma = L L^T in float64
// (right-looking, in LDS), X = L^-1 by forward substitution (one thread per
// column) and A = L^-T = X^T. A non-positive or non-finite pivot leaves the
// metric as it was (counted in counters[1] when count). The statistics are
// reset (from_stats) and every chain's dual averaging restarts from eps_bar
// (restart): eps = eps_bar, mu = ln(10 eps), h_bar = 0.
template <class T>
__global__ __launch_bounds__(256) void hmc_dense_window_kernel(
    int D, long long C, int from_stats, long long n, double reg, double jitter_cfg, double* __restrict__ s1,
    double* __restrict__ S2, const double* __restrict__ sig_in, double* __restrict__ minv64,
    double* __restrict__ a64, T* __restrict__ minvT, T* __restrict__ atT, long long* __restrict__ counters,
    int count, int restart, T* __restrict__ eps, const T* __restrict__ eps_bar, T* __restrict__ h_bar,
    T* __restrict__ mu) {
  __shared__ double Sg[64 * 64];  // Sigma
  __shared__ double Lm[64 * 64];  // lower + diagonal: L; strictly upper: A (= X^T)
  __shared__ double xd[64];       // diagonal of X = 1 / L_ii
  __shared__ int fail;
  const int tid = threadIdx.x;
  if (tid == 0) fail = 0;
  const double fl = jitter_cfg > 1e-10 ? jitter_cfg : 1e-10;
  const double nd = (double)n;
  for (int idx = tid; idx < D * D; idx += 256) {
    const int i = idx / D, j = idx - i * D;
    double v;
    if (from_stats) {
      const double s = (S2[idx] - s1[i] * s1[j] / nd) / (nd - 1.0);
      v = (1.0 - reg) * s + (i == j ? reg : 0.0);
      if (i == j) v = (v < fl) ? fl : v;
    } else {
      v = sig_in[idx];
    }
    Sg[idx] = v;
    Lm[idx] = v;
  }
  __syncthreads();
  for (int k = 0; k < D; ++k) {
    if (tid == 0) {
      const double piv = Lm[k * D + k];
      if (!(piv > 0.0) || !(piv < __builtin_inf())) fail = 1;
      else Lm[k * D + k] = __builtin_sqrt(piv);
    }
    __syncthreads();
    if (fail) break;  // block-uniform: read after the barrier
    const double lkk = Lm[k * D + k];
    __syncthreads();
    for (int i = k + 1 + tid; i < D; i += 256) Lm[i * D + k] = Lm[i * D + k] / lkk;
    __syncthreads();
    const int m = D - k - 1;
    for (int idx = tid; idx < m * m; idx += 256) {
      const int i = k + 1 + idx / m, j = k + 1 + idx % m;
      if (j <= i) Lm[i * D + j] = Lm[i * D + j] - Lm[i * D + k] * Lm[j * D + k];
    }
    __syncthreads();
  }
  const bool ok = !fail;
  if (ok) {
    if (tid < D) {  // column tid of X = L^-1, stored as row tid of the strictly upper part
      const int j = tid;
      const double xjj = 1.0 / Lm[j * D + j];
      xd[j] = xjj;
      for (int i = j + 1; i < D; ++i) {
        double s = Lm[i * D + j] * xjj;
        for (int k = j + 1; k < i; ++k) s += Lm[i * D + k] * Lm[j * D + k];
        Lm[j * D + i] = -s / Lm[i * D + i];
      }
    }
    __syncthreads();
    for (int idx = tid; idx < D * D; idx += 256) {
      const int i = idx / D, j = idx - i * D;
      const double a = (i < j) ? Lm[idx] : (i == j) ? xd[i] : 0.0;  // A_ij
      minv64[idx] = Sg[idx];
      minvT[idx] = (T)Sg[idx];
      a64[idx] = a;
      atT[j * D + i] = (T)a;
    }
  }
  if (tid == 0 && count) counters[ok ? 0 : 1] += 1;
  if (from_stats) {
    for (int idx = tid; idx < D * D; idx += 256) S2[idx] = 0.0;
    if (tid < D) s1[tid] = 0.0;
  }
  if (restart) {
    for (long long c = tid; c < C; c += 256) {
      const T e = eps_bar[c];
      eps[c] = e;
      mu[c] = glog((T)10 * e);
      h_bar[c] = (T)0;
    }
  }
}

hipError_t launch_hmc_dense_window(gm_dtype dt, int D, long long C, int from_stats, long long n, double reg,
                                   double jitter, double* s1, double* S2, const double* sig_in, double* minv64,
                                   double* a64, void* minvT, void* atT, long long* counters, int count, int restart,
                                   void* eps, const void* eps_bar, void* h_bar, void* mu, hipStream_t st) {
  if (dt == GM_F32)
    hipLaunchKernelGGL(hmc_dense_window_kernel<float>, dim3(1), dim3(256), 0, st, D, C, from_stats, n, reg, jitter,
                       s1, S2, sig_in, minv64, a64, (float*)minvT, (float*)atT, counters, count, restart,
                       (float*)eps, (const float*)eps_bar, (float*)h_bar, (float*)mu);
  else
    hipLaunchKernelGGL(hmc_dense_window_kernel<double>, dim3(1), dim3(256), 0, st, D, C, from_stats, n, reg, jitter,
                       s1, S2, sig_in, minv64, a64, (double*)minvT, (double*)atT, counters, count, restart,
                       (double*)eps, (const double*)eps_bar, (double*)h_bar, (double*)mu);
  return hipGetLastError();
}

}  // namespace gm
