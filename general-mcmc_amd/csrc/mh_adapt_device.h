// mh_adapt_device.h — the Metropolis-Hastings transition with a per-chain
// proposal scale and a per-chain diagonal proposal shape, and their warm-up
// adaptation (device code only; compiled ahead of time by
// mh_adapt_{f32,f64}_m{0,1,2}.hip and at run time for user targets by
// gm_jit.cpp). mh_kernel (mh_device.h) stays the path of every sampler that
// uses none of this; with equal scales and the all-ones shape this kernel
// returns its bits.
//
// One transition of chain c (T = sampler dtype; z, ln u: the draws of
// mh_kernel, same Philox streams, tags and counters):
//   f[i] = scale[c] * diag[c][i]     rounded to T once per (chain, coordinate, scale value)
//   y[i] = x[i] + z[i] * f[i]
//   log_alpha = lp(y) - lp(x);  accept iff log_alpha > ln u
// The proposal is symmetric, so its log q terms cancel: mh_kernel's `cancel`
// form, the only one here (the host admits only scales at which mh_kernel
// takes it, gmcmc_api.cpp mh_scale_ok).
//
// Shape convention: diag is a standard deviation per coordinate (the proposal
// is N(x, scale^2 diag^2)); the adapted diag is the square root of the
// regularised sample variance of the warm-up positions.
//
// MODE 0: frozen scale and shape. MODE 1: dual averaging of the scale after
// every transition on alpha = min(1, exp(log_alpha)) (the recurrence of
// hmc_adapt_device.h: gamma 0.05, t0 10, kappa 0.75), restart counter
// k = k0 + s + 1. MODE 2: MODE 1 plus the Welford update of (rmean, rm2) with
// the post-accept position while sb < m < lim. k, the Welford count and m are
// the same for every chain, so they are launch arguments; the host cuts
// launches at every window end and runs mh_adapt_window_kernel
// (mh_adapt_kernels.hip) between them. The dual-averaging state is computed
// from group-reduced values only, so it is identical in all lanes of a chain
// (wave-uniform at one chain per wave).
#pragma once
#include "gm_device.h"
#include "gm_launch.h"
#include "gm_track.h"

namespace gm {

template <class T, int LPC, int E, class TG, int MODE>
__global__ __launch_bounds__(256) void mh_adapt_kernel(MhAdaptLaunch aa, TG tg_) {
  const MhLaunch& a = aa.m;
  const long long gtid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long c = gtid / LPC;
  const int lane = (int)(gtid % LPC);
  const auto tg = tg_.template bind<LPC, E>(lane);  // per-lane target view
  // f64 proposals: the table-driven Box-Muller, as mh_kernel
  constexpr bool TAB = sizeof(T) == 8;
  __shared__ BmLds bm_lds[1];
  if constexpr (TAB) {
    bm_lds_fill(bm_lds[0]);
    __syncthreads();
  }
  if (c >= a.C) return;
  const int D = a.D;
  T* __restrict__ qs = (T*)a.q;
  const uint32_t cid = a.chain_offset + (uint32_t)c;
  const uint32_t ucid = (LPC == 64) ? (uint32_t)__builtin_amdgcn_readfirstlane((int)cid) : cid;
  // every lane of a chain holds the chain's scale (and, while adapting, the
  // same dual-averaging state)
  T sc = ((const T*)aa.scale)[c];

  T x[E], y[E], gdummy[E];
  // the proposal's factor scale * diag in registers; the shape itself only
  // where the scale changes (MODE >= 1). A frozen launch with 128 bytes of
  // factors per lane (f64 x 16, where mh_kernel already spills) re-reads the
  // shape from L2 every step instead and forms the same product: the same
  // bits, and no more scratch than mh_kernel has there.
  constexpr bool FMEM = MODE == 0 && sizeof(T) * E >= 128;
  T f[FMEM ? 1 : E], dg[MODE >= 1 ? E : 1];
  const T* __restrict__ dgp = aa.diag != nullptr ? (const T*)aa.diag + c * D : nullptr;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int i = lane * E + e;
    x[e] = (i < D) ? qs[c * D + i] : (T)0;
    const T d = (dgp != nullptr && i < D) ? dgp[i] : (T)1;
    if constexpr (MODE >= 1) dg[e] = d;
    if constexpr (!FMEM) f[e] = sc * d;
  }
  T sc_bar = (T)0, h_bar = (T)0, mu = (T)0;
  if constexpr (MODE >= 1) {
    sc_bar = ((const T*)aa.scale_bar)[c];
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
  T lp = tg.template eval<LPC, E, true>(x, gdummy, lane);
  long long acc = 0;
  NormalCache<T> ncache[E];  // f32: msun Box-Muller
  UniformCache<T> ucache;
  uint64_t lblk = ~0ull;  // LPC == 64: the 64-step window whose accept logs lnl holds (lane k: step 64 lblk + k)
  T lnl = (T)0;
  const bool track = a.trk.mean != nullptr;  // run_progress
  ChainTrack<LPC, E> tr;
  if (track) tr.load(a.trk, c, lane, D);
  const T gamma = (T)0.05, kappa = (T)0.75, delta = (T)aa.delta;
  // one step from x given its proposal normals z (+0 in padded slots, whose
  // y = +0 + +0 * f then stays +0)
  auto step = [&](int s, const T (&z)[E]) __attribute__((always_inline)) {
    const uint64_t st = a.step0 + (uint64_t)s;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if constexpr (FMEM) {
        const int i = lane * E + e;
        const T d = (dgp != nullptr && i < D) ? dgp[i] : (T)1;
        y[e] = x[e] + z[e] * (sc * d);
      } else {
        y[e] = x[e] + z[e] * f[e];
      }
    }
    const T lp1 = tg.finish(group_sum<LPC>(tg.template eval_part<LPC, E>(y, gdummy, lane)));
    const T log_alpha = lp1 - lp;
    T lnu;
    if constexpr (LPC == 64) {
      // the accept log-uniforms of 64 consecutive steps in one VALU pass, as
      // mh_kernel: a window boundary may fall anywhere in a launch
      constexpr int S = Blk<T>::S;
      const uint64_t b = st / 64;
      if (b != lblk) {
        const uint64_t sk = b * 64 + (uint64_t)lane;
        T us[S];
        uniforms_of(draw_block_v(a.seed, ucid, sk / S, TAG_MH_ACC, 0u), us);
        T um = us[0];
#pragma unroll
        for (int k = 1; k < S; ++k) um = ((lane & (S - 1)) == k) ? us[k] : um;
        lnl = glog_unif(um);
        lblk = b;
      }
      lnu = lane_k(lnl, (int)(st % 64));
    } else {
      lnu = glog_unif(ucache.get(a.seed, ucid, st, TAG_MH_ACC, 0u));
    }
    const bool accept = log_alpha > lnu;
    if (LPC == 64 ? (__builtin_amdgcn_readfirstlane((int)accept) != 0) : accept) {
#pragma unroll
      for (int e = 0; e < E; ++e) x[e] = y[e];
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
      sc = gexp(mu - gsqrt(kf) / gamma * h_bar);
      eta = gexp(-kappa * glog(kf));  // k^(-kappa)
      sc_bar = gexp(((T)1 - eta) * glog(sc_bar) + eta * glog(sc));
#pragma unroll
      for (int e = 0; e < E; ++e) f[e] = sc * dg[e];
      if constexpr (MODE == 2) {
        const long long m = aa.m0 + s + 1;
        if (m > aa.sb && m < aa.lim) {  // the arithmetic of hmc_adapt_kernel's Welford update
          rn += 1;
          const T ns = (T)rn;
#pragma unroll
          for (int e = 0; e < E; ++e) {
            const T d1 = x[e] - rmean[e];
            rmean[e] = rmean[e] + d1 / ns;
            const T d2 = x[e] - rmean[e];
            rm2[e] = rm2[e] + d1 * d2;
          }
        }
      }
    }
    if (track) tr.step(x, a.trk.n0 + (unsigned long long)s + 1ull, lane, D);
    if (s >= a.collect_from) {
      T* __restrict__ out = (T*)a.samples + ((a.sample_row0 + (s - a.collect_from)) * a.C + c) * D;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int i = lane * E + e;
        if (i < D) out[i] = x[e];
      }
    }
  };
  if constexpr (TAB) {
    // f64: one Philox block and Box-Muller pair per coordinate serve the steps
    // st = 2b (z0) and 2b + 1 (z1), the lane's E blocks and pairs issued side
    // by side, as mh_kernel. A launch that starts at an odd step (a window
    // end cut the pair) takes z1 alone.
    for (int s = 0; s < a.n_steps;) {
      const uint64_t st = a.step0 + (uint64_t)s;
      u32x4 w[E];
      double z0[E], z1[E];
      draw_blocks_v<E>(w, a.seed, cid, st / 2, TAG_MH_PROP, (uint32_t)(lane * E));
      normals_tab_n<E>(w, z0, z1, bm_lds[0]);
      if (D < LPC * E) {  // padded slots (wave-uniform): their normals +0
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const bool in = lane * E + e < D;
          z0[e] = in ? z0[e] : 0.0;
          z1[e] = in ? z1[e] : 0.0;
        }
      }
      if ((st & 1u) == 0) {
        step(s, z0);
        ++s;
      }
      if (s < a.n_steps) {
        step(s, z1);
        ++s;
      }
    }
  } else {
    for (int s = 0; s < a.n_steps; ++s) {
      const uint64_t st = a.step0 + (uint64_t)s;
      T z[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int i = lane * E + e;
        z[e] = (i < D) ? ncache[e].get(a.seed, cid, st, TAG_MH_PROP, (uint32_t)i) : (T)0;
      }
      step(s, z);
    }
  }
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int i = lane * E + e;
    if (i < D) qs[c * D + i] = x[e];
    if constexpr (MODE == 2) {
      if (i < D) {
        ((T*)aa.rmean)[c * D + i] = rmean[e];
        ((T*)aa.rm2)[c * D + i] = rm2[e];
      }
    }
  }
  if (track) tr.store(a.trk, c, lane, D);
  if (lane == 0) {
    ((T*)a.logp)[c] = lp;
    a.accepts[c] += acc;
    if constexpr (MODE >= 1) {
      ((T*)aa.scale)[c] = sc;
      ((T*)aa.scale_bar)[c] = sc_bar;
      ((T*)aa.h_bar)[c] = h_bar;
    }
  }
}

}  // namespace gm
