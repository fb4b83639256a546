// hmc_dense_device.h — the HMC transition with a per-chain step size and ONE
// dense metric shared by all chains of the sampler (device code only;
// compiled ahead of time by hmc_dense_{f32,f64}_m{0,1}.hip). hmc_kernel
// (hmc_device.h) and hmc_adapt_kernel (hmc_adapt_device.h) stay the paths of
// every sampler that uses none of this; with the identity metric this kernel
// returns hmc_kernel's bits, with a diagonal metric of powers of four
// hmc_adapt_kernel's.
//
// Metric convention (Stan's): M^-1 = Sigma, the regularised covariance of the
// warm-up positions pooled over all chains; Sigma = L L^T, A = L^-T (upper
// triangular). One transition (T = sampler dtype; z, K0, ln u: the draws of
// hmc_kernel, same Philox streams, tags and counters):
//   p_i = sum_{j} A_ij z_j      (fma chain in ascending j from +0; A_ij = 0 for j < i
//                                adds zeros, so the chain is the one over j >= i)
//   K0 = 0.5 * sum z^2          (= 0.5 p' Sigma p)
//   L leapfrogs:  p += (eps/2) g;  v = Sigma p (fma chain, ascending j, from +0);
//                 q += eps v;  (logp, g) = target(q);  p += (eps/2) g
//   K1 = 0.5 * sum_i p_i v_i with v = Sigma p of the final p
//   accept iff (logp' - logp) + (K0 - K1) >= ln u   (NaN rejects)
// Kicks and drift are single fused multiply-adds.
//
// Sigma is wave-uniform: it is staged once per block in LDS as [D][S]
// (S = LPC * E, zero past D), after the target's own staging area; the vector
// of a product is broadcast through a per-lane-group LDS slot, as the dense
// Gaussian target's product does (gm_device.h GaussLane::eval_impl). A is read
// from global memory (L2-resident) where a draw block is filled, once per
// Blk<T>::S transitions.
//
// User targets (gm_jit.cpp) run one chain per lane, LPC = 1 and E = D: the
// "group" is the lane itself and its slot holds the lane's own vector, which
// the runtime index j of the chain reads back (a register array could only be
// indexed by a fully unrolled D x D product). There the slots are laid out
// [S][blockDim.x], element j of lane t at j * blockDim.x + t, so that a wave's
// reads of one j fall in consecutive banks; hmc_dense_lds_user (gm_launch.h)
// gives the bytes and hmc_dense_user_block the block size that keeps the
// workgroup within 64 KiB.
//
// MODE 0: frozen step size. MODE 1: dual averaging of the step size after
// every transition, with the recurrences and constants of hmc_adapt_device.h.
// The pooled statistics of the warm-up are not taken here: the warm-up
// launches store their post-accept positions through the sample-store path
// and hmc_dense_kernels.hip accumulates them between launches.
#pragma once
#include "gm_device.h"
#include "gm_launch.h"

namespace gm {

// dynamic LDS bytes of the metric for layout (LPC, E) in a 256-thread block:
// Sigma [D][S] and one slot [S] per lane group
template <class T, int LPC, int E> __host__ __device__ constexpr size_t hmc_dense_lds(int D) {
  return ((size_t)D * LPC * E + (size_t)256 * E) * sizeof(T);
}
__host__ __device__ constexpr size_t hmc_dense_align(size_t b) { return (b + 15) & ~(size_t)15; }
static_assert(sizeof(BmLds32) == HMC_DENSE_LDS_STATIC, "the kernel's static LDS (gm_launch.h)");

template <class T, int LPC, int E, class TG, int MODE>
__global__ __launch_bounds__(256) void hmc_dense_kernel(HmcDenseLaunch aa, TG tg_) {
  const HmcLaunch& a = aa.h;
  const long long gtid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long c = gtid / LPC;
  const int lane = (int)(gtid % LPC);
  const auto tg = tg_.template bind<LPC, E>(lane);  // per-lane target view (stages its own LDS)
  __shared__ BmLds32 bm32[1];  // f32 momenta: the table-driven Box-Muller, as hmc_kernel
  if constexpr (sizeof(T) == 4) bm_lds_fill32(bm32[0]);
  const int D = a.D;
  constexpr int S = LPC * E;
  // the metric's LDS region sits after the target's own
  T* const sm = (T*)(gm_dyn_lds + hmc_dense_align(tg_.template lds_bytes<LPC, E>()));
  {
    const T* __restrict__ mg = (const T*)aa.minv;
    const int n = D * S;
    for (int k = threadIdx.x; k < n; k += blockDim.x) {
      const int j = k / S, i = k - j * S;
      sm[k] = (i < D) ? mg[j * D + i] : (T)0;
    }
  }
  __syncthreads();
  if (c >= a.C) return;  // whole lane groups leave together
  // this lane group's slot; element j is sd[j * SJ]
  const int SJ = (LPC == 1) ? (int)blockDim.x : 1;
  T* const sd = sm + D * S + ((LPC == 1) ? (int)threadIdx.x : (int)(threadIdx.x / LPC) * S);
  const T* const smr = sm + lane * E;
  T* __restrict__ qs = (T*)a.q;
  T eps = ((const T*)aa.eps)[c];
  T half = (T)0.5 * eps;
  const uint32_t cid = a.chain_offset + (uint32_t)c;
  const uint32_t ucid = (LPC == 64) ? (uint32_t)__builtin_amdgcn_readfirstlane((int)cid) : cid;

  // the lane group's vector x through the slot (the previous product's reads
  // are done before it is replaced)
  auto publish = [&](const T (&x)[E]) __attribute__((always_inline)) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int e = 0; e < E; ++e) sd[(lane * E + e) * SJ] = x[e];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  // w = Sigma x: fma chain in ascending j from +0 (rows past D are zero)
  auto sigma_mv = [&](const T (&x)[E], T (&w)[E]) __attribute__((always_inline)) {
    publish(x);
#pragma unroll
    for (int e = 0; e < E; ++e) w[e] = (T)0;
#pragma unroll 4
    for (int j = 0; j < D; ++j) {
      const T xj = sd[j * SJ];
#pragma unroll
      for (int e = 0; e < E; ++e) w[e] = gfma(smr[j * S + e], xj, w[e]);
    }
  };

  T q[E], g[E], p[E], q1[E], p1[E], g1[E], v[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int i = lane * E + e;
    q[e] = (i < D) ? qs[c * D + i] : (T)0;
  }
  T eps_bar = (T)0, h_bar = (T)0, mu = (T)0;
  if constexpr (MODE >= 1) {
    eps_bar = ((const T*)aa.eps_bar)[c];
    h_bar = ((const T*)aa.h_bar)[c];
    mu = ((const T*)aa.mu)[c];
  }
  T lp = tg.template eval<LPC, E, true>(q, g, lane);
  long long acc = 0;
  constexpr int SB = Blk<T>::S;  // one Philox block serves SB transitions
  const PhiloxKeys pk = philox_keys(a.seed);
  // draw blocks A (current) and B (prefetched on the wave's phase), as hmc_kernel
  T zsA[E][SB], kesA[SB], lusA[SB];
  T zsB[E][SB], kesB[SB], lusB[SB];
  bool hasB = false;
  const int phase = (int)((gtid >> 6) % SB);
  const T* __restrict__ atg = (const T*)aa.at;
  auto fill = [&](T (&zs)[E][SB], T (&kes)[SB], T (&lus)[SB], uint64_t blk) __attribute__((always_inline)) {
    // the block holds the momenta p = A z, not the normals; K0 = 0.5 sum z^2
    // (= 0.5 p' Sigma p) is summed from z before the product, in hmc_kernel's order
    T kp[SB];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int i = lane * E + e;
      momenta_of(draw_block(pk, cid, blk, TAG_MOM, (uint32_t)i), zs[e], bm32[0]);
#pragma unroll
      for (int k = 0; k < SB; ++k) {
        const T z = (i < D) ? zs[e][k] : (T)0;
        const T sq = z * z;
        kp[k] = (e == 0) ? sq : kp[k] + sq;
        zs[e][k] = z;
      }
    }
    group_sum_n<LPC>(kp);
#pragma unroll
    for (int k = 0; k < SB; ++k) kes[k] = kp[k] * (T)0.5;
#pragma unroll
    for (int k = 0; k < SB; ++k) {
      T z[E], w[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        z[e] = zs[e][k];
        w[e] = (T)0;
      }
      publish(z);
#pragma unroll 4
      for (int j = 0; j < D; ++j) {
        const T zj = sd[j * SJ];
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const int i = lane * E + e;
          const T aij = (i < D) ? atg[j * D + i] : (T)0;
          w[e] = gfma(aij, zj, w[e]);
        }
      }
#pragma unroll
      for (int e = 0; e < E; ++e) zs[e][k] = w[e];
    }
    T us[SB];
    uniforms_of(draw_block(a.seed, ucid, blk, TAG_ACC, 0u), us);
    if constexpr (LPC == 64) {
      T um = us[0];
#pragma unroll
      for (int k = 1; k < SB; ++k) um = ((lane & (SB - 1)) == k) ? us[k] : um;
      const T lm = glog_unif(um);
#pragma unroll
      for (int k = 0; k < SB; ++k) lus[k] = lane_k(lm, k);
    } else {
#pragma unroll
      for (int k = 0; k < SB; ++k) lus[k] = glog_unif(us[k]);
    }
  };
  const uint64_t st_end = a.step0 + (uint64_t)a.n_steps;
  T* __restrict__ out = (T*)a.samples + (a.sample_row0 * a.C + c) * D + lane * E;
  const long long row_stride = a.C * D;
  const T gamma = (T)0.05, kappa = (T)0.75, delta = (T)aa.delta;

  for (int s = 0; s < a.n_steps; ++s) {
    const uint64_t st = a.step0 + (uint64_t)s;
    const int k0 = (int)(st % SB);
    if (s == 0 || k0 == 0) {
      if (s > 0 && hasB) {
#pragma unroll
        for (int k = 0; k < SB; ++k) {
#pragma unroll
          for (int e = 0; e < E; ++e) zsA[e][k] = zsB[e][k];
          kesA[k] = kesB[k];
          lusA[k] = lusB[k];
        }
      } else {
        fill(zsA, kesA, lusA, st / SB);
#pragma unroll
        for (int e = 0; e < E; ++e) skip_front(zsA[e], k0);
        skip_front(kesA, k0);
        skip_front(lusA, k0);
      }
      hasB = false;
    }
    // 1. momentum p = A z ~ N(0, M): front of the block
#pragma unroll
    for (int e = 0; e < E; ++e) {
      p[e] = zsA[e][0];
      shift_front(zsA[e]);
    }
    const T ke0 = kesA[0];
    const T lnu = lusA[0];
    shift_front(kesA);
    shift_front(lusA);
    if (!hasB && k0 == phase && st - (uint64_t)k0 + SB < st_end) {
      fill(zsB, kesB, lusB, st / SB + 1);
      hasB = true;
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
      q1[e] = q[e];
      p1[e] = p[e];
      g1[e] = g[e];
    }
    // 5. leapfrog; the drift is q += eps (Sigma p)
    T lp1 = lp;
    auto kick = [&]() __attribute__((always_inline)) {
#pragma unroll
      for (int e = 0; e < E; ++e) p1[e] = gfma(g1[e], half, p1[e]);
    };
    auto drift = [&]() __attribute__((always_inline)) {
      sigma_mv(p1, v);
#pragma unroll
      for (int e = 0; e < E; ++e) q1[e] = gfma(v[e], eps, q1[e]);
    };
    auto lf = [&]() __attribute__((always_inline)) {
      kick();
      drift();
      tg.template eval<LPC, E, false>(q1, g1, lane);
      kick();
    };
    int l = 0;
    if (a.lf_unroll == 4)
      for (; l + 4 < a.L; l += 4) { lf(); lf(); lf(); lf(); }
    if (a.lf_unroll == 2)
      for (; l + 2 < a.L; l += 2) { lf(); lf(); }
    for (; l + 1 < a.L; ++l) lf();
    // 6. proposed kinetic energy: in-lane sums of p' v in coordinate order, v = Sigma p'
    auto kin_part = [&]() __attribute__((always_inline)) {
      sigma_mv(p1, v);
      T kq = (T)0;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const T sq = p1[e] * v[e];
        kq = (e == 0) ? sq : kq + sq;
      }
      return kq;
    };
    T ke1;
    if (a.L >= 1) {
      kick();
      drift();
      using TL = typename Bare<decltype(tg)>::type;
      if constexpr (requires { TL::template has_part<LPC>; }) {
        if constexpr (TL::template has_part<LPC>) {
          T sums[2];
          sums[0] = tg.template eval_part<LPC, E>(q1, g1, lane);
          kick();
          sums[1] = kin_part();
          group_sum_n<LPC>(sums);
          lp1 = tg.finish(sums[0]);
          ke1 = sums[1] * (T)0.5;
        } else {
          lp1 = tg.template eval<LPC, E, true>(q1, g1, lane);
          kick();
          ke1 = group_sum<LPC>(kin_part()) * (T)0.5;
        }
      } else {
        lp1 = tg.template eval<LPC, E, true>(q1, g1, lane);
        kick();
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
