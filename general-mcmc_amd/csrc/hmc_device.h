// hmc_device.h — the HMC transition kernels (device code only). hmc_kernel is
// compiled ahead of time by hmc_f32.hip and hmc_f64.hip (hmc_part.inc, one
// translation unit per dtype so that they build in parallel), hmc_wide_kernel
// by hmc_kernels.hip, and hmc_kernel at run time for user targets by
// gm_jit.cpp. The algorithm notes are at the top of hmc_kernels.hip, which
// also holds launch_hmc, the one entry point of all three. The draw-wave
// form of hmc_kernel's block form is hmc_dw_kernel (hmc_dw_device.h).
#pragma once
#include "gm_device.h"
#include "gm_launch.h"

namespace gm {

#ifndef GM_LF_U
#define GM_LF_U GM_LF_LONG  // (measurement builds: the long form's trip length)
#endif
#ifndef GM_LF_BU
#define GM_LF_BU GM_LF_BLOCK  // (measurement builds: the block form's pass length)
#endif

// a compile-time index handed to a generic lambda, and f(IntC<K>) for K < S
template <int V> struct IntC { static constexpr int v = V; };
template <int K, int S, class F> __device__ __forceinline__ void for_each_k(F&& f) {
  if constexpr (K < S) {
    f(IntC<K>{});
    for_each_k<K + 1, S>(f);
  }
}
// f(IntC<P>) for the powers of two P = 1 << B, 1 << (B + 1), ... below U
template <int B, int U, class F> __device__ __forceinline__ void for_each_pow2_below(F&& f) {
  if constexpr ((1 << B) < U) {
    f(IntC<(1 << B)>{});
    for_each_pow2_below<B + 1, U>(f);
  }
}

// One chain per wave: the accept log-uniforms of the 64-transition window that
// holds draw block blk, lane k's the one of transition 64 w + k (stream
// TAG_ACC, index 0: block (64 w + k) / S, word k % S, as every transition's
// own draw). One per-lane Philox and one glog_unif pass serve 64 transitions
// (as mh_kernel's, mh_device.h); per block, all 64 lanes ran that pass for S
// distinct values behind a scalar Philox.
template <class T>
__device__ __forceinline__ T accept_window(uint64_t seed, uint32_t ucid, uint64_t blk, int lane) {
  constexpr int S = Blk<T>::S;
  // the window's first block has its low log2(64 / S) bits clear: no carry
  const uint64_t lb = (blk & ~(uint64_t)(64 / S - 1)) | (uint64_t)(lane / S);
  T us[S];
  uniforms_of(draw_block_v(seed, ucid, lb, TAG_ACC, 0u), us);
  T um = us[0];
#pragma unroll
  for (int k = 1; k < S; ++k) um = ((lane & (S - 1)) == k) ? us[k] : um;
  return glog_unif(um);
}

// LF: the leapfrog loop form (1, 2 or 4 leapfrogs per trip, or GM_LF_LONG: the
// long count-down form) as a constant, or 0 for the launch's a.lf_unroll (the
// forms 1, 2 and 4 in the code; GM_LF_LONG and GM_LF_BLOCK then run as 1),
// or GM_LF_BLOCK: the block form (hmc_block_part.inc).
//
// One chain per wave (LPC = 64): the per-chain sums of a transition are left
// in row 3 of the wave (lanes 48..63, group_sum_n_row3) and everything derived
// from them (the kinetic energies, log_alpha, the chain's logp) is computed
// there in the vector registers, without the read of lane 63 into a scalar
// and back. The accept log-uniforms of the 64 transitions 64 w .. 64 w + 63
// (a window) sit in the 64 lanes of one register, computed in one VALU pass
// per window (accept_window); transition st reads lane st % 64 of it as a
// scalar, the decision is bit 63 of one vector compare with it, and the
// branch on it is wave-uniform. The accept count and the sample row pointer
// are then scalars.
template <class T, int LPC, int E, class TG, int LF = 0>
__global__ __launch_bounds__(256) void hmc_kernel(HmcLaunch a, TG tg_) {
  constexpr bool W1 = LPC == 64;
  const long long gtid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long c = gtid / LPC;
  const int lane = (int)(gtid % LPC);
  const auto tg = tg_.template bind<LPC, E>(lane);  // per-lane target view
  // f32 momenta: the table-driven Box-Muller (gm_rng.h normals_tab32); its
  // tables in LDS, filled by the whole block before any thread returns
  __shared__ BmLds32 bm32[1];
  if constexpr (sizeof(T) == 4) {
    bm_lds_fill32(bm32[0]);
    __syncthreads();
  }
  if (c >= a.C) return;  // whole lane groups leave together
  const int D = a.D;
  T* __restrict__ qs = (T*)a.q;
  const T eps = (T)a.eps;
  const T half = (T)0.5 * eps;  // batched_hmc.rs:167
  const uint32_t cid = a.chain_offset + (uint32_t)c;
  // wave-uniform chain id when one chain fills the wave: the per-chain draws
  // (accept uniform) then run on the scalar unit
  const uint32_t ucid = (LPC == 64) ? (uint32_t)__builtin_amdgcn_readfirstlane((int)cid) : cid;

  T q[E], g[E], q1[E], p1[E], g1[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int i = lane * E + e;
    q[e] = (i < D) ? qs[c * D + i] : (T)0;
  }
  T lp = tg.template eval<LPC, E, true>(q, g, lane);
  long long acc = 0;
  constexpr int S = Blk<T>::S;  // one Philox block serves S transitions
  const PhiloxKeys pk = philox_keys(a.seed);  // momentum streams' round keys, in VGPRs
  // Draw blocks: A = the current block, B = the next one, prefetched. The
  // transition loop below is unrolled over the position k inside a block, so
  // slot k of A is a fixed register at each place that reads it (nothing is
  // shifted or indexed at run time). Each wave prefetches at the position
  // that matches its wave phase, so the waves of a SIMD are not all in the
  // Philox/Box-Muller chain at once and the leapfrogs of the others hide its
  // latency. W1: the lus are unused; lw is the accept window of block A (lane
  // k: ln u of transition 64 w + k) and lwN the next window, which the
  // prefetch of a window's first block computes (at this wave's phase
  // position like the rest of the block, so the waves of a SIMD do not take
  // the pass at the same transition) and the A <- B copy of that block hands
  // over. A launch's first fill computes its whole window, wherever it starts.
  T zsA[E][S], kesA[S], lusA[S];
  T zsB[E][S], kesB[S], lusB[S];
  T lw = (T)0, lwN = (T)0;
  // wave index mod S, as a scalar (every lane of a wave has the same value)
  const int phase = __builtin_amdgcn_readfirstlane((int)((gtid >> 6) % S));
  // the momenta of block blk, their S kinetic energies (S independent
  // reductions) and the S accept log-uniforms (W1: block blk's window into
  // win, if `window`)
  auto fill = [&](T (&zs)[E][S], T (&kes)[S], T (&lus)[S], T& win, bool window, uint64_t blk)
                  __attribute__((always_inline)) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int i = lane * E + e;
      momenta_of(draw_block(pk, cid, blk, TAG_MOM, (uint32_t)i), zs[e], bm32[0]);
#pragma unroll
      for (int k = 0; k < S; ++k) zs[e][k] = (i < D) ? zs[e][k] : (T)0;
    }
    T kp[S];
#pragma unroll
    for (int k = 0; k < S; ++k) {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const T sq = zs[e][k] * zs[e][k];
        kp[k] = (e == 0) ? sq : kp[k] + sq;
      }
    }
    // 2. kinetic energies, the S sums interleaved (W1: totals in row 3)
    if constexpr (W1) group_sum_n_row3(kp);
    else group_sum_n<LPC>(kp);
#pragma unroll
    for (int k = 0; k < S; ++k) kes[k] = kp[k] * (T)0.5;
    if constexpr (W1) {
      if (window) win = accept_window<T>(a.seed, ucid, blk, lane);
    } else {
      T us[S];
      uniforms_of(draw_block(a.seed, ucid, blk, TAG_ACC, 0u), us);
#pragma unroll
      for (int k = 0; k < S; ++k) lus[k] = glog_unif(us[k]);
    }
  };
  // block b is the first of its accept window
  auto opens_window = [](uint64_t b) { return (b & (uint64_t)(64 / S - 1)) == 0; };
  const uint64_t st_end = a.step0 + (uint64_t)a.n_steps;
  // the first sample slot; each stored transition advances it one row (C*D
  // elements) instead of recomputing the 64-bit row address. W1: the chain's
  // row as a scalar pointer, the lane's offset added by the store itself.
  const long long cu =
      W1 ? (long long)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : c;
  // (D read back as a scalar of its own: the compiler otherwise shares the
  // 64-bit D of the per-lane state addresses, a vector register pair, and
  // the whole pointer chain follows it to the vector unit)
  const long long Du = W1 ? (long long)__builtin_amdgcn_readfirstlane(D) : (long long)D;
  T* __restrict__ out = (T*)a.samples + (a.sample_row0 * a.C + cu) * Du + (W1 ? 0 : lane * E);
  const long long row_stride = a.C * Du;
  const int lfu = LF ? LF : a.lf_unroll;
  uint32_t soff = (uint32_t)(lane * E * (int)sizeof(T));  // W1: byte offset of this lane's slots in a sample row

  int s = 0;             // transitions done
  uint64_t blk = 0;      // the draw block in A
  bool more = false;     // this launch reaches block blk + 1
  bool hasB = false;     // ... and B holds it
  // the transition at position K of block blk
  auto step = [&](auto kc) __attribute__((always_inline)) {
    constexpr int K = decltype(kc)::v;
    // 1. momentum ~ N(0, I) and its kinetic energy: slot K of the block;
    // 4. proposal buffers
#pragma unroll
    for (int e = 0; e < E; ++e) {
      q1[e] = q[e];
      p1[e] = zsA[e][K];
      g1[e] = g[e];
    }
    const T ke0 = kesA[K];
    // prefetch the next block (if this launch reaches it)
#ifdef GM_MEASURE_REUSE_DRAWS
    // (measurement builds only, never shipped: no draw block after the
    // launch's first, block A reused; wrong numbers, the time without fill)
    if (false) {
#else
    if (K == phase && more) {
#endif
      fill(zsB, kesB, lusB, lwN, opens_window(blk + 1), blk + 1);
      hasB = true;
    }
    // 5. leapfrog: L-1 gradient-only steps, then the last one with logp.
    // The kicks p + g*(eps/2) and the drift q + p*eps are the engine's fused
    // multiply-adds (one rounding each; the reference's tensor ops round the
    // product and the sum separately, batched_hmc.rs:166-190): 9 VALU per
    // 64-lane Rosenbrock leapfrog instead of 11 (+9 % headline,
    // profiles/r04/ab_hmc_fma_kick_drift.log); the oracle's engine form is
    // the same (gm_oracle_t.inc hmc_chains, form 0).
    T lp1 = lp;
    // (unrolled by hand: the DPP intrinsics are convergent, so the compiler
    // will not runtime-unroll, and a taken branch costs a wave ~20 cycles)
    auto lf = [&]() __attribute__((always_inline)) {
#pragma unroll
      for (int e = 0; e < E; ++e) p1[e] = gfma(g1[e], half, p1[e]);
#pragma unroll
      for (int e = 0; e < E; ++e) q1[e] = gfma(p1[e], eps, q1[e]);
      tg.template eval<LPC, E, false>(q1, g1, lane);
#pragma unroll
      for (int e = 0; e < E; ++e) p1[e] = gfma(g1[e], half, p1[e]);
    };
    // The block form: count-down passes of GM_LF_BU straight-line leapfrogs,
    // nothing scalar between them (L = 50: one pass), after the
    // (L - 1) % GM_LF_BU others as a binary ladder of straight-line pieces of
    // 1, 2, 4, ... leapfrogs, one wave-uniform bit test each, the whole ladder
    // skipped when there is no remainder. (A switch into one block, entered
    // at the position that leaves the remainder, is what this stands for: the
    // compiler makes the fall-through of that switch a flag test and a branch
    // in front of every leapfrog, profiles/r11/README.md.)
    if constexpr (LF == GM_LF_BLOCK) {
      const unsigned n1 = (unsigned)(a.L > 1 ? a.L - 1 : 0);
      int passes = (int)(n1 / (unsigned)GM_LF_BU);
      const int r = (int)n1 - passes * GM_LF_BU;
      auto lfs = [&](auto nc) __attribute__((always_inline)) {
        for_each_k<0, decltype(nc)::v>([&](auto) __attribute__((always_inline)) { lf(); });
      };
      if (r > 0)
        for_each_pow2_below<0, GM_LF_BU>([&](auto pc) __attribute__((always_inline)) {
          if (r & decltype(pc)::v) lfs(pc);
        });
      for (; passes > 0; --passes) lfs(IntC<GM_LF_BU>{});
    } else if constexpr (LF == GM_LF_LONG) {
      // The long form: single steps bring L - 1 to a multiple of GM_LF_LONG
      // (none at L = 50), then count-down trips of GM_LF_LONG straight-line
      // leapfrogs: one scalar decrement, compare and taken branch per trip and
      // no remainder test in it (7 taken branches per 49 leapfrogs where the x2
      // form has 25, and 3 scalar instructions per 7 leapfrogs for 5 per 2).
      const int n1 = a.L - 1;
      int trips = n1 > 0 ? (int)((unsigned)n1 / (unsigned)GM_LF_U) : 0;
      for (int r = n1 - trips * GM_LF_U; r > 0; --r) lf();
      for (; trips > 0; --trips) for_each_k<0, GM_LF_U>([&](auto) __attribute__((always_inline)) { lf(); });
    } else {
      int l = 0;
      if (lfu == 4)
        for (; l + 4 < a.L; l += 4) { lf(); lf(); lf(); lf(); }
      // two leapfrogs per loop trip at 2-4 waves per SIMD (one taken branch and
      // loop test per two): kernel -1.4 % at the headline's 4 waves per SIMD,
      // but cfg4 at 8 waves per SIMD -4.7 % (profiles/r04/ab_hmc_unroll2.log)
      if (lfu == 2)
        for (; l + 2 < a.L; l += 2) { lf(); lf(); }
      for (; l + 1 < a.L; ++l) lf();
    }
    // 6. proposed kinetic energy, from the in-lane sums of p'^2
    auto kin_part = [&]() __attribute__((always_inline)) {
      T kq = (T)0;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const T sq = p1[e] * p1[e];
        kq = (e == 0) ? sq : kq + sq;
      }
      return kq;
    };
    T ke1;
    if (a.L >= 1) {
#pragma unroll
      for (int e = 0; e < E; ++e) p1[e] = gfma(g1[e], half, p1[e]);
#pragma unroll
      for (int e = 0; e < E; ++e) q1[e] = gfma(p1[e], eps, q1[e]);
      using TL = typename Bare<decltype(tg)>::type;  // the per-lane target view
      if constexpr (requires { TL::template has_part<LPC>; }) {
        if constexpr (TL::template has_part<LPC>) {
          // the log-density and kinetic-energy sums reduced together
          T sums[2];
          sums[0] = tg.template eval_part<LPC, E>(q1, g1, lane);
#pragma unroll
          for (int e = 0; e < E; ++e) p1[e] = gfma(g1[e], half, p1[e]);
          sums[1] = kin_part();
          if constexpr (W1) group_sum_n_row3(sums);
          else group_sum_n<LPC>(sums);
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
    // 7-9. Metropolis accept (NaN log_alpha rejects). W1: the operands are
    // the chain's in row 3; this transition's ln u is its lane of the window,
    // read as a scalar, and lane 63's compare decides
    const T log_alpha = (lp1 - lp) + (ke0 - ke1);
    bool accept;
    if constexpr (W1) {
      const T lnu = lane_k(lw, (int)(((uint32_t)blk * (uint32_t)S + (uint32_t)K) & 63u));
      // (bit 31 of the mask's high word, opaque as a scalar: the compiler
      // turns a test of bit 63 of the 64-bit mask into a signed 64-bit
      // compare, which only the vector unit has)
      uint32_t hi = (uint32_t)(__builtin_amdgcn_ballot_w64(log_alpha >= lnu) >> 32);
      asm volatile("" : "+s"(hi));
      accept = (hi >> 31) != 0;
    } else {
      accept = log_alpha >= lusA[K];
    }
    if (accept) {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        q[e] = q1[e];
        g[e] = g1[e];
      }
      lp = lp1;
      ++acc;
    }
    if (s >= a.collect_from) {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int i = lane * E + e;
        // W1: scalar row pointer + this lane's 32-bit byte offset (the saddr
        // store form). The empty asm on the offset's own register keeps its
        // zero extension next to the store, where instruction selection can
        // fold it (hoisted out of the loop it becomes a 64-bit add per row);
        // in place, so it costs no move.
        if constexpr (W1) {
          if (e == 0) asm volatile("" : "+v"(soff));
          if (i < D) *(T*)((char*)out + soff + e * sizeof(T)) = q[e];
        } else {
          if (i < D) out[e] = q[e];
        }
      }
      out += row_stride;
    }
  };
  // Block by block, the S positions unrolled. A launch may start and end
  // inside a block (step0 % S, st_end % S): wave-uniform tests skip the
  // positions before its first and after its last transition.
  if (a.n_steps > 0) {
    blk = a.step0 / S;
    int kb = (int)(a.step0 % S);
    for (;;) {
      if (hasB) {
#pragma unroll
        for (int k = 0; k < S; ++k) {
#pragma unroll
          for (int e = 0; e < E; ++e) zsA[e][k] = zsB[e][k];
          kesA[k] = kesB[k];
          if (!W1) lusA[k] = lusB[k];
        }
        if constexpr (W1) {
          if (opens_window(blk)) lw = lwN;
        }
#ifdef GM_MEASURE_REUSE_DRAWS
      } else if (s == 0) {
#else
      } else {
#endif
        // the launch's first block, or the one after a first block that began
        // past this wave's prefetch position (its window is already in lw
        // unless it opens a new one)
        fill(zsA, kesA, lusA, lw, s == 0 || opens_window(blk), blk);
      }
      hasB = false;
      more = (blk + 1) * S < st_end;
      for_each_k<0, S>([&](auto kc) __attribute__((always_inline)) {
        if (decltype(kc)::v >= kb && s < a.n_steps) {
          step(kc);
          ++s;
        }
      });
      if (!more) break;
      kb = 0;
      ++blk;
    }
  }
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int i = lane * E + e;
    if (i < D) qs[c * D + i] = q[e];
  }
  // W1: lane 63 owns the chain's logp (row 3)
  if (lane == (W1 ? 63 : 0)) {
    ((T*)a.logp)[c] = lp;
    a.accepts[c] += acc;
  }
}

// ---------------------------------------------------------------------------
// hmc_wide_kernel: the same transition for dim > 1024, one chain per
// workgroup of W = blockDim/64 waves (WideCtx in gm_device.h). The per-step
// momenta of a draw block (S transitions) go to a per-chain scratch in HBM
// (each thread re-reads only what it wrote), the accept log-uniforms stay in
// registers; every per-chain sum is a block reduction, so the accept branch is
// uniform over the workgroup. The reference's 10,000-dimensional Rosenbrock
// benchmark (hmc.rs:757-791) runs here.
template <class T, int E, class TG>
__global__ __launch_bounds__(gm_wide_max_threads(sizeof(T), E)) void hmc_wide_kernel(HmcLaunch a, TG tg_) {
  __shared__ T xf[2 * GM_WIDE_MAX_WAVES], xl[2 * GM_WIDE_MAX_WAVES], red[GM_WIDE_MAX_WAVES];
  const int tid = threadIdx.x;
  const long long c = blockIdx.x;
  const auto tg = tg_.template bind<64, E>(tid);  // coordinates tid*E + e
  __shared__ BmLds32 bm32[1];  // f32 momenta: the table-driven Box-Muller
  if constexpr (sizeof(T) == 4) {
    bm_lds_fill32(bm32[0]);
    __syncthreads();
  }
  WideCtx<T> cx{tid >> 6, (int)(blockDim.x >> 6), tid & 63, xf, xl, red, 0};
  const int D = a.D;
  const long long Dp = (long long)blockDim.x * E;
  T* __restrict__ qs = (T*)a.q;
  const T eps = (T)a.eps;
  const T half = (T)0.5 * eps;
  const uint32_t cid = a.chain_offset + (uint32_t)c;
  constexpr int S = Blk<T>::S;
  T* __restrict__ zs = (T*)a.zs + c * S * Dp;
  // q: current position; g1: the gradient at q1, which is the current
  // position at every transition start (a rejected proposal re-evaluates the
  // gradient at q instead of keeping a copy: same bits, E fewer registers)
  T q[E], q1[E], p1[E], g1[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int i = tid * E + e;
    q[e] = (i < D) ? qs[c * D + i] : (T)0;
  }
  T lp = tg.template eval_wide<E, true>(q, g1, cx);
#pragma unroll
  for (int e = 0; e < E; ++e) q1[e] = q[e];
  long long acc = 0;
  T lus[S];
  for (int s = 0; s < a.n_steps; ++s) {
    const uint64_t st = a.step0 + (uint64_t)s;
    const int k0 = (int)(st % S);
    if (s == 0 || k0 == 0) {  // draw block st/S: momenta to scratch, accept logs to registers
#pragma unroll 1
      for (int e = 0; e < E; ++e) {
        const int i = tid * E + e;
        T z[S];
        momenta_of(draw_block(a.seed, cid, st / S, TAG_MOM, (uint32_t)i), z, bm32[0]);
#pragma unroll
        for (int k = 0; k < S; ++k) zs[k * Dp + i] = (i < D) ? z[k] : (T)0;
      }
      T us[S];
      uniforms_of(draw_block(a.seed, cid, st / S, TAG_ACC, 0u), us);
#pragma unroll
      for (int k = 0; k < S; ++k) lus[k] = glog_unif(us[k]);
    }
    // 1-2. momentum ~ N(0, I) and its kinetic energy
    T kp = (T)0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      p1[e] = zs[k0 * Dp + tid * E + e];
      const T sq = p1[e] * p1[e];
      kp = (e == 0) ? sq : kp + sq;
    }
    const T ke0 = block_sum(kp, cx) * (T)0.5;
    T lnu = lus[0];
#pragma unroll
    for (int k = 1; k < S; ++k) lnu = (k0 == k) ? lus[k] : lnu;
    // 4-5. proposal and leapfrog (q1 = q and g1 = grad(q) here)
    T lp1 = lp;
    for (int l = 0; l < a.L; ++l) {
#pragma unroll
      for (int e = 0; e < E; ++e) p1[e] = gfma(g1[e], half, p1[e]);
#pragma unroll
      for (int e = 0; e < E; ++e) q1[e] = gfma(p1[e], eps, q1[e]);
      if (l + 1 < a.L) tg.template eval_wide<E, false>(q1, g1, cx);
      else lp1 = tg.template eval_wide<E, true>(q1, g1, cx);
#pragma unroll
      for (int e = 0; e < E; ++e) p1[e] = gfma(g1[e], half, p1[e]);
    }
    // 6. proposed kinetic energy
    T kq = (T)0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const T sq = p1[e] * p1[e];
      kq = (e == 0) ? sq : kq + sq;
    }
    const T ke1 = block_sum(kq, cx) * (T)0.5;
    // 7-9. Metropolis accept (NaN log_alpha rejects); block-uniform
    const T log_alpha = (lp1 - lp) + (ke0 - ke1);
    if (log_alpha >= lnu) {
#pragma unroll
      for (int e = 0; e < E; ++e) q[e] = q1[e];
      lp = lp1;
      ++acc;
    } else {
#pragma unroll
      for (int e = 0; e < E; ++e) q1[e] = q[e];
      if (a.L > 0) tg.template eval_wide<E, false>(q1, g1, cx);
    }
    if (s >= a.collect_from) {
      T* __restrict__ out = (T*)a.samples + ((a.sample_row0 + (s - a.collect_from)) * a.C + c) * D;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int i = tid * E + e;
        if (i < D) out[i] = q[e];
      }
    }
  }
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int i = tid * E + e;
    if (i < D) qs[c * D + i] = q[e];
  }
  if (tid == 0) {
    ((T*)a.logp)[c] = lp;
    a.accepts[c] += acc;
  }
}

}  // namespace gm
