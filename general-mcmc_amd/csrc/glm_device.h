// glm_device.h — generalised linear model with canonical link and an
// independent Gaussian prior as a target (GM_TARGET_GLM): Bayesian logistic
// and Poisson regression on a data set of N rows by D columns shared by all
// chains. The chain's position is the coefficient vector theta.
//
//   eta_n = offset_n + sum_j X[n][j] theta_j
//   logp  = sum_n ( y_n eta_n - A(eta_n) ) - 0.5 sum_j theta_j^2 / s_j^2
//   g_j   = sum_n X[n][j] ( y_n - mu(eta_n) ) - theta_j / s_j^2
//   Bernoulli-logit: A = max(eta, 0) + log1p(exp(-|eta|)), mu = logistic(eta)
//   Poisson-log:     A = mu = exp(eta)
//
// Evaluation form. The LPC lanes of a chain split the ROWS: with RV = 16 /
// sizeof(T) rows per 16-byte vector, lane l owns the row vectors v with
// v mod LPC == l, i.e. rows RV*v .. RV*v + RV-1. X is stored transposed and
// zero-padded, xt[j*Np + n] (Np a multiple of 256, Dp = D rounded up to
// GLM_CH), so the lanes of a chain read one column of consecutive row vectors
// at consecutive addresses through the caches; the padding rows are masked out
// of the sums, the padding columns are zero.
//  1. theta is published to the group's LDS slot and read back as broadcasts.
//  2. Per row: eta = fma chain over ascending j from offset_n; the link; the
//     log-density term and the residual r_n = y_n - mu_n.
//  3. A gradient partial of GLM_CH columns, acc_k = fma(X[n][k], r_n, acc_k)
//     over the lane's rows in ascending n. With D > GLM_CH the columns are
//     taken in chunks of GLM_CH and the rows are walked once per chunk (eta
//     recomputed, the same operations, so the same bits): 2*D registers of
//     partials would spill.
//  4. The partials are reduce-scattered through the wave's LDS scratch,
//     glm_xc<T>() columns at a time: every lane writes its partials, the lane
//     that owns coordinate j sums the group's LPC partials of column j in
//     ascending lane order starting from lane 0's.
//  5. g_j = sum - theta_j * (1/s_j^2); the owner adds -0.5 theta_j^2 (1/s_j^2)
//     to its log-density part, slots in ascending order; padded slots get +0.
//  6. The log-density parts go through group_sum (eval) or are returned
//     unreduced (eval_part / finish) to be reduced with the kinetic energy.
// No atomics; nothing depends on the chain's place in the grid beyond its lane
// number in the group; every LDS exchange is inside one wave (a group is at
// most 64 lanes) and uses only the group's own region, so groups of a wave
// that NUTS runs under divergent control flow do not meet.
#pragma once
#include "../../include/gmcmc.h"
#include "gm_device.h"

namespace gm {

constexpr int GLM_CH = 32;        // gradient columns accumulated per pass over the rows
constexpr int GLM_MAX_DIM = 128;  // (gmcmc_api.cpp refuses more)
constexpr int GLM_ROW_PAD = 256;  // Np: rows padded to a multiple of LPC * RV for every layout
// columns per LDS exchange; the scratch row stride XC + 1 keeps the lanes'
// writes in different banks
template <class T> __host__ __device__ constexpr int glm_xc() { return sizeof(T) == 4 ? 16 : 8; }

__device__ __forceinline__ float glm_log1p(float v) { return ::log1pf(v); }
__device__ __forceinline__ double glm_log1p(double v) { return ::log1p(v); }

template <class T, int LPC, int E> struct GlmLane;
template <class T> struct GlmT {
  const T* xt;   // [Dp][Np] device, transposed and zero-padded
  const T* y;    // [Np] (0 past N)
  const T* off;  // [Np] (0 past N, all 0 without an offset)
  const T* iv;   // [Dp] 1 / prior_sd^2 (0 past D)
  long long N, Np;
  int D, Dp, family;
  // dynamic LDS bytes of a 256-thread block: the groups' theta slots, then
  // the exchange scratch (one row of XC + 1 per thread)
  template <int LPC, int E> __host__ __device__ static constexpr size_t lds_need() {
    return ((size_t)256 * E + (size_t)256 * (glm_xc<T>() + 1)) * sizeof(T);
  }
  template <int LPC, int E> __host__ __device__ size_t lds_bytes() const { return lds_need<LPC, E>(); }
  template <int LPC, int E> __device__ __forceinline__ GlmLane<T, LPC, E> bind(int lane) const {
    static_assert(LPC <= 64 && (LPC * E) % GLM_CH == 0, "GLM layouts: one wave, whole column chunks");
    GlmLane<T, LPC, E> r;
    r.xt = xt;
    r.y = y;
    r.off = off;
    r.N = N;
    r.Np = Np;
    r.D = D;
    r.Dp = Dp;
    r.family = family;
#pragma unroll
    for (int e = 0; e < E; ++e) r.ivr[e] = (lane * E + e < D) ? iv[lane * E + e] : (T)0;
    T* base = (T*)gm_dyn_lds;
    const int t = (int)threadIdx.x;
    r.sth = base + (t / LPC) * (LPC * E);
    r.sxg = base + 256 * E + (t - lane) * (glm_xc<T>() + 1);
    return r;
  }
};

template <class T, int LPC, int E> struct GlmLane {
  static constexpr int RV = 16 / (int)sizeof(T);  // rows per 16-byte vector
  static constexpr int XC = glm_xc<T>();
  typedef T vR __attribute__((ext_vector_type(16 / sizeof(T))));
  const T* xt;
  const T* y;
  const T* off;
  long long N, Np;
  int D, Dp, family;
  T ivr[E];  // this lane's 1 / prior_sd^2 (0 past D)
  T* sth;    // LDS: the group's theta [LPC * E]
  T* sxg;    // LDS: the group's exchange scratch, LPC rows of XC + 1

  template <int LPC_> static constexpr bool has_part = true;
  template <int LPC_, int E_>
  __device__ __forceinline__ T eval_part(const T (&x)[E], T (&g)[E], int lane) const {
    return eval_impl<LPC_, E_, true>(x, g, lane);
  }
  __device__ __forceinline__ T finish(T total) const { return total; }
  template <int LPC_, int E_, bool LOGP>
  __device__ __forceinline__ T eval(const T (&x)[E], T (&g)[E], int lane) const {
    const T part = eval_impl<LPC_, E_, LOGP>(x, g, lane);
    if (LOGP) return group_sum<LPC>(part);
    return (T)0;
  }

  // mu(eta) and, with LOGP, A(eta)
  template <bool LOGP> __device__ __forceinline__ void link(T eta, T& mu, T& A) const {
    if (family == GM_GLM_POISSON_LOG) {
      mu = gexp(eta);
      A = mu;
    } else {
      const T ae = eta < (T)0 ? -eta : eta;
      const T em = gexp(-ae);  // in (0, 1]; 0 once |eta| passes the exp range
      const T den = (T)1 + em;
      mu = (eta >= (T)0 ? (T)1 : em) / den;
      if (LOGP) A = (eta > (T)0 ? eta : (T)0) + glm_log1p(em);
    }
  }

  template <int LPC_, int E_, bool LOGP>
  __device__ __forceinline__ T eval_impl(const T (&x)[E], T (&g)[E], int lane) const {
    static_assert(LPC_ == LPC && E_ == E, "layout mismatch");
    // the previous evaluation's broadcast reads are done before theta is replaced
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int e = 0; e < E; ++e) sth[lane * E + e] = (lane * E + e < D) ? x[e] : (T)0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    T part = (T)0;
    T gs[E];
#pragma unroll
    for (int e = 0; e < E; ++e) gs[e] = (T)0;
    constexpr int JB = 8;  // columns whose loads are in flight together
    for (int c0 = 0; c0 < Dp; c0 += GLM_CH) {
      T acc[GLM_CH];
#pragma unroll
      for (int k = 0; k < GLM_CH; ++k) acc[k] = (T)0;
      for (long long n0 = (long long)lane * RV; n0 < Np; n0 += (long long)LPC * RV) {
        const T* xp = xt + n0;
        const vR ov = *(const vR*)(off + n0);
        const vR yv = *(const vR*)(y + n0);
        T eta[RV];
#pragma unroll
        for (int u = 0; u < RV; ++u) eta[u] = ov[u];
        for (int j0 = 0; j0 < Dp; j0 += JB) {
          vR xv[JB];
          T th[JB];
#pragma unroll
          for (int k = 0; k < JB; ++k) xv[k] = *(const vR*)(xp + (long long)(j0 + k) * Np);
#pragma unroll
          for (int k = 0; k < JB; ++k) th[k] = sth[j0 + k];
#pragma unroll
          for (int k = 0; k < JB; ++k) {
#pragma unroll
            for (int u = 0; u < RV; ++u) eta[u] = gfma(xv[k][u], th[k], eta[u]);
          }
        }
        T r[RV];
#pragma unroll
        for (int u = 0; u < RV; ++u) {
          const bool valid = n0 + u < N;
          T mu, A = (T)0;
          link<LOGP>(eta[u], mu, A);
          r[u] = valid ? yv[u] - mu : (T)0;
          if (LOGP && c0 == 0) {
            const T term = valid ? yv[u] * eta[u] - A : (T)0;
            part = part + term;
          }
        }
#pragma unroll
        for (int k0 = 0; k0 < GLM_CH; k0 += JB) {
          vR xv[JB];
#pragma unroll
          for (int k = 0; k < JB; ++k) xv[k] = *(const vR*)(xp + (long long)(c0 + k0 + k) * Np);
#pragma unroll
          for (int k = 0; k < JB; ++k) {
#pragma unroll
            for (int u = 0; u < RV; ++u) acc[k0 + k] = gfma(xv[k][u], r[u], acc[k0 + k]);
          }
          // one batch of loads in flight at a time: without it the scheduler
          // hoists all GLM_CH column loads of the unrolled loop (GLM_CH * 16
          // bytes of registers per lane) and the kernels drop to one wave per SIMD
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      // reduce-scatter of the chunk's partials, XC columns at a time
      T* mine = sxg + lane * (XC + 1);
#pragma unroll
      for (int x0 = 0; x0 < GLM_CH; x0 += XC) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 0; k < XC; ++k) mine[k] = acc[x0 + k];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const int rel = lane * E + e - (c0 + x0);
          if (rel >= 0 && rel < XC) {
            T s = sxg[rel];
#pragma unroll 8
            for (int l = 1; l < LPC; ++l) s = s + sxg[l * (XC + 1) + rel];
            gs[e] = s;
          }
        }
      }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const bool in = lane * E + e < D;
      const T pv = x[e] * ivr[e];
      g[e] = in ? gs[e] - pv : (T)0;
      if (LOGP) part = part - (in ? ((T)0.5 * x[e]) * pv : (T)0);
    }
    return part;
  }
};

}  // namespace gm
