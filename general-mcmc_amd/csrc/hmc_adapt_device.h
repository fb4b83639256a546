// hmc_adapt_device.h — the HMC transition with a per-chain step size and a
// per-chain diagonal metric, and their warm-up adaptation (device code only;
// compiled ahead of time by hmc_adapt_{f32,f64}_m{0,1,2}.hip and at run
// time for user targets by gm_jit.cpp). hmc_kernel (hmc_device.h) stays the
// path of every sampler that uses none of this; with equal step sizes and the
// identity metric this kernel returns its bits.
//
// One transition (T = sampler dtype; z, K0, ln u: the draws of hmc_kernel,
// same Philox streams, tags and counters):
//   p = dsq * z;   K0 = 0.5 * sum z^2
//   L leapfrogs:  p += (eps/2) g;  q += (eps*dinv) * p;  (logp, g) = target(q);  p += (eps/2) g
//   K1 = 0.5 * sum dinv * p^2;  log_alpha = (logp' - logp) + (K0 - K1);  accept iff log_alpha >= ln u
// dinv = M^-1, dsq = sqrt(M) = 1/sqrt(dinv). Kicks and drift are single fused
// multiply-adds; eps*dinv is rounded to T once per chain, coordinate and
// step-size value.
//
// Metric convention: the adapted M^-1 is the regularised sample VARIANCE of
// the warm-up positions (as in Stan and PyMC). The NUTS path of this library
// follows the reference text instead and stores inv = 1/var
// (nuts_kernels.hip diag_from_var); the two are deliberately different and
// NUTS is not changed.
//
// MODE 0: frozen step size and metric. MODE 1: dual averaging of the step
// size after every transition (gamma 0.05, t0 10, kappa 0.75: the constants
// of nuts_device.h), restart counter k = k0 + s + 1. MODE 2: MODE 1 plus the
// Welford update of (rmean, rm2) with the post-accept position while
// sb < m < lim. k, the Welford count and m are the same for every chain (the
// window schedule depends on the transition index only), so they are launch
// arguments; the host cuts launches at every window end and runs
// hmc_adapt_window_kernel (hmc_adapt_kernels.hip) between them.
#pragma once
#include "gm_device.h"
#include "gm_launch.h"

namespace gm {

template <class T, int LPC, int E, class TG, int MODE>
__global__ __launch_bounds__(256) void hmc_adapt_kernel(HmcAdaptLaunch aa, TG tg_) {
  const HmcLaunch& a = aa.h;
  const long long gtid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long c = gtid / LPC;
  const int lane = (int)(gtid % LPC);
  const auto tg = tg_.template bind<LPC, E>(lane);  // per-lane target view
  __shared__ BmLds32 bm32[1];  // f32 momenta: the table-driven Box-Muller, as hmc_kernel
  if constexpr (sizeof(T) == 4) {
    bm_lds_fill32(bm32[0]);
    __syncthreads();
  }
  if (c >= a.C) return;  // whole lane groups leave together
  const int D = a.D;
  T* __restrict__ qs = (T*)a.q;
  // every lane of a chain holds the chain's step size (and, while adapting,
  // the same dual-averaging state: the recurrences run on group-reduced
  // values, identical in all lanes of the chain)
  T eps = ((const T*)aa.eps)[c];
  T half = (T)0.5 * eps;
  const uint32_t cid = a.chain_offset + (uint32_t)c;
  const uint32_t ucid = (LPC == 64) ? (uint32_t)__builtin_amdgcn_readfirstlane((int)cid) : cid;

  T q[E], g[E], p[E], q1[E], p1[E], g1[E];
  // the metric: M^-1 and eps*M^-1 in registers; sqrt(M) is re-read where a
  // draw block is filled (once per S transitions, L2-resident)
  T dinv[E], epsd[E];
  const T* __restrict__ dsqp = (const T*)aa.dsq + c * D;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int i = lane * E + e;
    q[e] = (i < D) ? qs[c * D + i] : (T)0;
    dinv[e] = (i < D) ? ((const T*)aa.dinv)[c * D + i] : (T)0;
    epsd[e] = eps * dinv[e];
  }
  T eps_bar = (T)0, h_bar = (T)0, mu = (T)0;
  if constexpr (MODE >= 1) {
    eps_bar = ((const T*)aa.eps_bar)[c];
    h_bar = ((const T*)aa.h_bar)[c];
    mu = ((const T*)aa.mu)[c];
  }
  T rmean[MODE == 2 ? E : 1], rm2[MODE == 2 ? E : 1];
  long long rn = aa.rn0;
  if constexpr (MODE == 2) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int i = lane * E + e;
      rmean[e] = (i < D) ? ((const T*)aa.rmean)[c * D + i] : (T)0;
      rm2[e] = (i < D) ? ((const T*)aa.rm2)[c * D + i] : (T)0;
    }
  }
  T lp = tg.template eval<LPC, E, true>(q, g, lane);
  long long acc = 0;
  constexpr int S = Blk<T>::S;  // one Philox block serves S transitions
  const PhiloxKeys pk = philox_keys(a.seed);
  // draw blocks A (current) and B (prefetched on the wave's phase), as hmc_kernel
  T zsA[E][S], kesA[S], lusA[S];
  T zsB[E][S], kesB[S], lusB[S];
  bool hasB = false;
  const int phase = (int)((gtid >> 6) % S);
  auto fill = [&](T (&zs)[E][S], T (&kes)[S], T (&lus)[S], uint64_t blk) __attribute__((always_inline)) {
    // the block holds the momenta p = sqrt(M) z, not the normals: sqrt(M) is
    // read here, once per block and under the Philox/Box-Muller latency, and
    // K0 = 0.5 sum z^2 (= 0.5 p' M^-1 p) is summed from z before the scaling,
    // in hmc_kernel's order
    T kp[S];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int i = lane * E + e;
      const T sm = (i < D) ? dsqp[i] : (T)0;
      momenta_of(draw_block(pk, cid, blk, TAG_MOM, (uint32_t)i), zs[e], bm32[0]);
#pragma unroll
      for (int k = 0; k < S; ++k) {
        const T z = (i < D) ? zs[e][k] : (T)0;
        const T sq = z * z;
        kp[k] = (e == 0) ? sq : kp[k] + sq;
        zs[e][k] = sm * z;
      }
    }
    group_sum_n<LPC>(kp);
#pragma unroll
    for (int k = 0; k < S; ++k) kes[k] = kp[k] * (T)0.5;
    T us[S];
    uniforms_of(draw_block(a.seed, ucid, blk, TAG_ACC, 0u), us);
    if constexpr (LPC == 64) {
      T um = us[0];
#pragma unroll
      for (int k = 1; k < S; ++k) um = ((lane & (S - 1)) == k) ? us[k] : um;
      const T lm = glog_unif(um);
#pragma unroll
      for (int k = 0; k < S; ++k) lus[k] = lane_k(lm, k);
    } else {
#pragma unroll
      for (int k = 0; k < S; ++k) lus[k] = glog_unif(us[k]);
    }
  };
  const uint64_t st_end = a.step0 + (uint64_t)a.n_steps;
  T* __restrict__ out = (T*)a.samples + (a.sample_row0 * a.C + c) * D + lane * E;
  const long long row_stride = a.C * D;
  const T gamma = (T)0.05, kappa = (T)0.75, delta = (T)aa.delta;

  for (int s = 0; s < a.n_steps; ++s) {
    const uint64_t st = a.step0 + (uint64_t)s;
    const int k0 = (int)(st % S);
    if (s == 0 || k0 == 0) {
      if (s > 0 && hasB) {
#pragma unroll
        for (int k = 0; k < S; ++k) {
#pragma unroll
          for (int e = 0; e < E; ++e) zsA[e][k] = zsB[e][k];
          kesA[k] = kesB[k];
          lusA[k] = lusB[k];
        }
      } else {
        fill(zsA, kesA, lusA, st / S);
#pragma unroll
        for (int e = 0; e < E; ++e) skip_front(zsA[e], k0);
        skip_front(kesA, k0);
        skip_front(lusA, k0);
      }
      hasB = false;
    }
    // 1. momentum p = sqrt(M) z ~ N(0, M): front of the block
#pragma unroll
    for (int e = 0; e < E; ++e) {
      p[e] = zsA[e][0];
      shift_front(zsA[e]);
    }
    const T ke0 = kesA[0];
    const T lnu = lusA[0];
    shift_front(kesA);
    shift_front(lusA);
    if (!hasB && k0 == phase && st - (uint64_t)k0 + S < st_end) {
      fill(zsB, kesB, lusB, st / S + 1);
      hasB = true;
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
      q1[e] = q[e];
      p1[e] = p[e];
      g1[e] = g[e];
    }
    // 5. leapfrog; the drift's factor is eps*dinv[e]
    T lp1 = lp;
    auto lf = [&]() __attribute__((always_inline)) {
#pragma unroll
      for (int e = 0; e < E; ++e) p1[e] = gfma(g1[e], half, p1[e]);
#pragma unroll
      for (int e = 0; e < E; ++e) q1[e] = gfma(p1[e], epsd[e], q1[e]);
      tg.template eval<LPC, E, false>(q1, g1, lane);
#pragma unroll
      for (int e = 0; e < E; ++e) p1[e] = gfma(g1[e], half, p1[e]);
    };
    int l = 0;
    if (a.lf_unroll == 4)
      for (; l + 4 < a.L; l += 4) { lf(); lf(); lf(); lf(); }
    if (a.lf_unroll == 2)
      for (; l + 2 < a.L; l += 2) { lf(); lf(); }
    for (; l + 1 < a.L; ++l) lf();
    // 6. proposed kinetic energy: in-lane sums of dinv p'^2 in coordinate order
    auto kin_part = [&]() __attribute__((always_inline)) {
      T kq = (T)0;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const T sq = (p1[e] * p1[e]) * dinv[e];
        kq = (e == 0) ? sq : kq + sq;
      }
      return kq;
    };
    T ke1;
    if (a.L >= 1) {
#pragma unroll
      for (int e = 0; e < E; ++e) p1[e] = gfma(g1[e], half, p1[e]);
#pragma unroll
      for (int e = 0; e < E; ++e) q1[e] = gfma(p1[e], epsd[e], q1[e]);
      using TL = typename Bare<decltype(tg)>::type;
      if constexpr (requires { TL::template has_part<LPC>; }) {
        if constexpr (TL::template has_part<LPC>) {
          T sums[2];
          sums[0] = tg.template eval_part<LPC, E>(q1, g1, lane);
#pragma unroll
          for (int e = 0; e < E; ++e) p1[e] = gfma(g1[e], half, p1[e]);
          sums[1] = kin_part();
          group_sum_n<LPC>(sums);
          lp1 = tg.finish(sums[0]);
          ke1 = sums[1] * (T)0.5;
        } else {
          lp1 = tg.template eval<LPC, E, true>(q1, g1, lane);
#pragma unroll
          for (int e = 0; e < E; ++e) p1[e] = gfma(g1[e], half, p1[e]);
          ke1 = group_sum<LPC>(kin_part()) * (T)0.5;
        }
      } else {
        lp1 = tg.template eval<LPC, E, true>(q1, g1, lane);
#pragma unroll
        for (int e = 0; e < E; ++e) p1[e] = gfma(g1[e], half, p1[e]);
        ke1 = group_sum<LPC>(kin_part()) * (T)0.5;
      }
    } else {
      ke1 = group_sum<LPC>(kin_part()) * (T)0.5;
    }
    // 7-9. Metropolis accept (NaN log_alpha rejects)
    const T log_alpha = (lp1 - lp) + (ke0 - ke1);
    // the transition's record (gm_launch.h StatsRec), before lp and eps move on
    if (aa.stats.rec != nullptr && lane == 0) {
      T al = gexp(log_alpha);
      al = al > (T)1 ? (T)1 : al;
      al = (al == al) ? al : (T)0;
      stats_store<T>(aa.stats, a.C, c, s, ke0 - lp, al, eps,
                     stats_word(a.L, 0, !(log_alpha > (T)-1000), log_alpha >= lnu));
    }
    if (log_alpha >= lnu) {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        q[e] = q1[e];
        g[e] = g1[e];
      }
      lp = lp1;
      ++acc;
    }
    if constexpr (MODE >= 1) {
      // dual averaging on alpha = min(1, exp(log_alpha)), NaN -> 0
      T al = gexp(log_alpha);
      al = al > (T)1 ? (T)1 : al;
      al = (al == al) ? al : (T)0;
      const T kf = (T)(aa.k0 + s + 1);
      T eta = (T)1 / (kf + (T)10);
      h_bar = ((T)1 - eta) * h_bar + eta * (delta - al);
      eps = gexp(mu - gsqrt(kf) / gamma * h_bar);
      eta = gexp(-kappa * glog(kf));  // k^(-kappa)
      eps_bar = gexp(((T)1 - eta) * glog(eps_bar) + eta * glog(eps));
      half = (T)0.5 * eps;
#pragma unroll
      for (int e = 0; e < E; ++e) epsd[e] = eps * dinv[e];
      if constexpr (MODE == 2) {
        const long long m = aa.m0 + s + 1;
        if (m > aa.sb && m < aa.lim) {  // the arithmetic of the NUTS warm-up's RunningCov::update
          rn += 1;
          const T ns = (T)rn;
#pragma unroll
          for (int e = 0; e < E; ++e) {
            const T d1 = q[e] - rmean[e];
            rmean[e] = rmean[e] + d1 / ns;
            const T d2 = q[e] - rmean[e];
            rm2[e] = rm2[e] + d1 * d2;
          }
        }
      }
    }
    if (s >= a.collect_from) {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int i = lane * E + e;
        if (i < D) out[e] = q[e];
      }
      out += row_stride;
    }
  }
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int i = lane * E + e;
    if (i < D) qs[c * D + i] = q[e];
    if constexpr (MODE == 2) {
      if (i < D) {
        ((T*)aa.rmean)[c * D + i] = rmean[e];
        ((T*)aa.rm2)[c * D + i] = rm2[e];
      }
    }
  }
  if (lane == 0) {
    ((T*)a.logp)[c] = lp;
    a.accepts[c] += acc;
    if constexpr (MODE >= 1) {
      ((T*)aa.eps)[c] = eps;
      ((T*)aa.eps_bar)[c] = eps_bar;
      ((T*)aa.h_bar)[c] = h_bar;
    }
  }
}

}  // namespace gm
