// glm_predict_device.h — posterior prediction of a GLM over stored draws
// (gm_glm_predict*, include/gmcmc.h). Not in the reference.
//
// Per draw s and data row m, in the draws' dtype T:
//   eta = offset_m + sum_j X[m][j] theta_sj
//   mu  = logistic(eta) | exp(eta)                  (the forms of GlmLane::link)
//   ll  = (y_m eta - A(eta)) + c_m
// and per row, reduced over all S draws in float64: mean and sd of eta and mu,
// mean and variance of ll, lppd = log((1/S) sum_s exp ll).
//
// Main kernel. eta is the product Theta X^T on the matrix cores
// (v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64): 16 draws are the A rows,
// 16 data rows the B columns, the accumulator starts at offset_m, the columns
// are zero-padded to the instantiation's KS k-steps of 4. A workgroup is four
// waves; wave w owns data rows 16 w .. 16 w + 15 of the workgroup's 64 and
// keeps their X fragments (KS registers a lane) for the whole launch. The
// workgroup walks the draws of its slab (GP_SLAB) in stages of GP_STAGE = 32:
// the stage's Theta goes through LDS in fragment order, every wave forms two
// independent 16 x 16 eta tiles from it, and each lane folds its 4 draws of
// one data row per tile into its running state:
//   eta, mu, ll:  pivot p (the lane's first value, 0 when that is not finite),
//                 sum (x - p), sum (x - p)^2                    float64
//   lppd:         running maximum m, sum exp(ll - m)            float64
// C/D maps: f32 draw = 4 (lane >> 4) + reg, f64 draw = (lane >> 4) + 4 reg;
// data row = lane & 15 in both.
// The four lane quarters of a wave hold different draws of the same rows: each
// writes its partial (n, sum, M2 of the three quantities, m, s) to
// part[slab][quarter][field][row].
//
// Merge kernel. One thread per row takes the partials in ascending (slab,
// quarter) order: sums added, M2 by Chan's formula, (m, s) by the max / scaled
// sum rule. No atomics. The split depends on (S, M, D, dtype) only.
#pragma once
#include "glm_device.h"

namespace gm {

constexpr int GP_SLAB = 8192;   // draws per slab
constexpr int GP_ROWS = 64;     // data rows per workgroup (4 waves x 16)
constexpr int GP_TILE = 16;     // draws per matrix-core tile
constexpr int GP_STAGE = 32;    // draws staged through LDS at a time (two tiles)
constexpr int GP_FIELDS = 9;    // n | eta sum, M2 | mu sum, M2 | ll sum, M2 | m | s
constexpr int GP_OUTS = 7;      // eta_mean, eta_sd, mu_mean, mu_sd, lppd, ll_mean, ll_var

template <class T> struct GlmPredictArgs {
  const T* x;      // [M][4 KS] zero-padded
  const T* off;    // [M]
  const T* y;      // [M] or null
  const T* c;      // [M] (with y)
  const T* draws;  // [S] rows of stride elements
  long long S, stride, M;
  int D, family;
  long long row0, rows;  // this launch's rows; rows_pad = 64 gridDim.y
  double* part;          // [slabs][4][GP_FIELDS][rows_pad]
  T* pw;                 // [S][M] or null
};

typedef float gp_f32x4 __attribute__((ext_vector_type(4)));
typedef double gp_f64x4 __attribute__((ext_vector_type(4)));
template <class T> struct GpAcc;
template <> struct GpAcc<float> {
  typedef gp_f32x4 type;
  static __device__ __forceinline__ type mma(float a, float b, type c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int draw(int q, int reg) { return 4 * q + reg; }
};
template <> struct GpAcc<double> {
  typedef gp_f64x4 type;
  static __device__ __forceinline__ type mma(double a, double b, type c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int draw(int q, int reg) { return q + 4 * reg; }
};

// mu(eta) and A(eta): GlmLane::link
template <class T> __device__ __forceinline__ void gp_link(int family, T eta, T& mu, T& A) {
  if (family == GM_GLM_POISSON_LOG) {
    mu = gexp(eta);
    A = mu;
  } else {
    const T ae = eta < (T)0 ? -eta : eta;
    const T em = gexp(-ae);
    const T den = (T)1 + em;
    mu = (eta >= (T)0 ? (T)1 : em) / den;
    A = (eta > (T)0 ? eta : (T)0) + glm_log1p(em);
  }
}

struct GpMoment {
  double p, s1, s2;
  __device__ __forceinline__ void add(bool first, double v) {
    if (first) p = (v - v == 0.0) ? v : 0.0;
    const double d = v - p;
    s1 = s1 + d;
    s2 = __builtin_fma(d, d, s2);
  }
  // sum and M2 of the n values
  __device__ __forceinline__ void close(int n, double& sum, double& m2) const {
    const double dn = (double)n;
    sum = __builtin_fma(dn, p, s1);
    const double v = s2 - s1 * s1 / dn;
    m2 = v < 0.0 ? 0.0 : v;  // (rounding of a vanishing spread; a NaN stays)
  }
};

template <class T, int KS> __global__ __launch_bounds__(256) void glm_predict_main(const GlmPredictArgs<T> a) {
  using Acc = GpAcc<T>;
  T* sth = (T*)gm_dyn_lds;  // [2 tiles][KS][64]: lane l of k-step ks holds theta[draw l & 15][4 ks + (l >> 4)]
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, r = lane & 15;
  constexpr int DP = 4 * KS;
  const long long s_begin = (long long)blockIdx.x * GP_SLAB;
  const long long s_end = a.S - s_begin < GP_SLAB ? a.S : s_begin + GP_SLAB;
  const long long lrow = (long long)blockIdx.y * GP_ROWS + wave * 16 + r;
  const long long m = a.row0 + lrow;
  const bool rowok = lrow < a.rows && m < a.M;
  const bool has_y = a.y != nullptr;

  T xb[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) xb[ks] = rowok ? a.x[m * DP + 4 * ks + q] : (T)0;
  const T off = rowok ? a.off[m] : (T)0;
  const T ym = rowok && has_y ? a.y[m] : (T)0;
  const T cm = rowok && has_y ? a.c[m] : (T)0;

  GpMoment e{0.0, 0.0, 0.0}, u{0.0, 0.0, 0.0}, l{0.0, 0.0, 0.0};
  double lm = -__builtin_inf(), ls = 0.0;
  int n = 0;

  for (long long s0 = s_begin; s0 < s_end; s0 += GP_STAGE) {
    __syncthreads();  // the previous stage's fragment reads are done
    for (int idx = tid; idx < GP_STAGE * DP; idx += 256) {
      const int dr = idx / DP, col = idx - dr * DP;
      const long long s = s0 + dr;
      const T v = (s < s_end && col < a.D) ? a.draws[s * a.stride + col] : (T)0;
      sth[((dr >> 4) * KS + (col >> 2)) * 64 + (col & 3) * 16 + (dr & 15)] = v;
    }
    __syncthreads();
    typename Acc::type acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[t][g] = off;
    const bool two = s0 + GP_TILE < s_end;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      acc[0] = Acc::mma(sth[ks * 64 + lane], xb[ks], acc[0]);
      if (two) acc[1] = Acc::mma(sth[(KS + ks) * 64 + lane], xb[ks], acc[1]);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (t == 1 && !two) break;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const long long s = s0 + t * GP_TILE + Acc::draw(q, g);
        if (s >= s_end) continue;
        const T eta = acc[t][g];
        T mu, A;
        gp_link<T>(a.family, eta, mu, A);
        const bool first = n == 0;
        ++n;
        e.add(first, (double)eta);
        u.add(first, (double)mu);
        if (has_y) {
          const T ll = (ym * eta - A) + cm;
          if (a.pw && rowok) a.pw[s * a.M + m] = ll;
          const double dl = (double)ll;
          l.add(first, dl);
          const double mn = dl > lm ? dl : lm;
          if (mn > -__builtin_inf() || dl != dl) {
            if (mn != lm) ls = ls * gexp(lm - mn);
            ls = ls + gexp(dl - mn);
          }
          lm = mn;
        }
      }
    }
  }

  const long long rows_pad = (long long)gridDim.y * GP_ROWS;
  double* pp = a.part + ((long long)blockIdx.x * 4 + q) * GP_FIELDS * rows_pad + lrow;
  double f[GP_FIELDS];
  f[0] = (double)n;
  if (n > 0) {
    e.close(n, f[1], f[2]);
    u.close(n, f[3], f[4]);
    l.close(n, f[5], f[6]);
  } else {
#pragma unroll
    for (int k = 1; k < 7; ++k) f[k] = 0.0;
  }
  f[7] = lm;
  f[8] = ls;
#pragma unroll
  for (int k = 0; k < GP_FIELDS; ++k) pp[k * rows_pad] = f[k];
}

// out [GP_OUTS][M] at rows row0 .. row0 + rows - 1
__global__ __launch_bounds__(256) void glm_predict_merge(const double* part, long long slabs, long long rows_pad,
                                                         long long row0, long long rows, long long M, long long S,
                                                         int has_y, double* out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows || row0 + i >= M) return;
  double n = 0.0, sum[3] = {0.0, 0.0, 0.0}, mean[3] = {0.0, 0.0, 0.0}, m2[3] = {0.0, 0.0, 0.0};
  double lm = -__builtin_inf(), ls = 0.0;
  for (long long p = 0; p < slabs * 4; ++p) {
    const double* pp = part + p * GP_FIELDS * rows_pad + i;
    const double nb = pp[0];
    if (nb == 0.0) continue;
    const double nn = n + nb;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (k == 2 && !has_y) break;
      const double sb = pp[(1 + 2 * k) * rows_pad], qb = pp[(2 + 2 * k) * rows_pad];
      const double mb = sb / nb;
      if (n == 0.0) {
        mean[k] = mb;
        m2[k] = qb;
      } else {
        const double d = mb - mean[k];
        mean[k] = mean[k] + d * (nb / nn);
        m2[k] = (m2[k] + qb) + (d * d) * (n * nb / nn);
      }
      sum[k] = sum[k] + sb;
    }
    if (has_y) {
      const double mb = pp[7 * rows_pad], sb = pp[8 * rows_pad];
      if (mb > lm) {
        ls = ls * gexp(lm - mb) + sb;
        lm = mb;
      } else if (mb > -__builtin_inf() || sb != sb) {
        ls = ls + sb * gexp(mb - lm);
      }
    }
    n = nn;
  }
  double* o = out + row0 + i;
  const double dS = (double)S;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double mu = sum[k] / dS, var = m2[k] / (dS - 1.0);
    const int om = k == 0 ? 0 : k == 1 ? 2 : 5;
    if (k == 2 && !has_y) break;
    o[om * M] = mu;
    o[(om + 1) * M] = k == 2 ? var : ::sqrt(var);
  }
  if (has_y) o[4 * M] = (lm + ::log(ls)) - ::log(dS);
}

}  // namespace gm
