// hmc_dw_device.h — the draw-wave form of the HMC transition kernel (device
// code only): hmc_kernel's one-chain-per-wave, one-element-per-lane block
// form (hmc_device.h, LF = GM_LF_BLOCK) with the momenta, their kinetic
// energies and the accept windows made by waves of their own.
//
// A workgroup is 4 chain waves (wave index w = 0..3, chain 4 blockIdx + w) and
// NDW draw waves (wave index 4..4 + NDW - 1; draw wave dw serves the chain
// waves w = dw, dw + NDW, ... below 4). Nothing a draw block holds depends on
// the chain's state (it is a function of seed, chain id and block number), so
// the draw waves make block b + 1 while the chain waves run the S transitions
// of block b, and the Philox / Box-Muller / reduction chain leaves the chain
// waves' critical path. The hand-over is through LDS, double-buffered:
// zs[b & 1], kes[b & 1] per block, and the accept window of block b in
// lw[(b / (64 / S)) & 1] (a window serves 64 / S blocks, so its buffer
// changes when the window does). Built at NDW = GM_DW_WAVES = 1: one draw
// wave, 320 threads (4 and 2 measured slower, profiles/r12).
//
// Synchronisation is one __syncthreads() per draw block and nothing else:
//   table fill; barrier (f32 only);
//   draw waves fill buffer 0 with the launch's first block; barrier;
//   per block i of the launch: chain waves run block i from buffer i & 1
//   while draw waves fill buffer (i + 1) & 1 if the launch has a block i + 1;
//   barrier.
// INVARIANT: the number of barriers a wave executes is (f32: 1) and, when
// a.n_steps > 0, 1 + nblk more, nblk = the draw blocks the launch touches: a
// function of a.step0 and a.n_steps alone, the same for every wave of the
// grid and both roles. No wave returns before its last barrier; a chain wave
// past a.C, and a draw wave for such a chain, runs the barrier sequence with
// its work switched off by a wave-uniform test.
//
// Every number is made by the same operations in the same order as in
// hmc_kernel: the draws, sums and transition below are its text at W1, E = 1
// over the shared pieces (draw_block, momenta_of, group_sum_n_row3,
// accept_window, the target's eval / eval_part, gfma).
#pragma once
#include "hmc_device.h"

namespace gm {

constexpr int GM_DW_CHAIN_WAVES = 4;

template <class T> struct DwLds {
  static constexpr int S = Blk<T>::S;
  T zs[2][GM_DW_CHAIN_WAVES][S][64];  // momenta of a block, zero past D
  T kes[2][GM_DW_CHAIN_WAVES][S];     // their kinetic energies
  T lw[2][GM_DW_CHAIN_WAVES][64];     // accept windows (lane k: ln u of transition 64 w + k)
};

template <class T, class TG, int NDW>
__global__ __launch_bounds__(64 * (GM_DW_CHAIN_WAVES + NDW)) void hmc_dw_kernel(HmcLaunch a, TG tg_) {
  static_assert(NDW == 1 || NDW == 2 || NDW == 4, "draw waves per workgroup");
  constexpr int S = Blk<T>::S;
  constexpr int CW = GM_DW_CHAIN_WAVES;
  constexpr uint64_t WB = 64 / S;  // draw blocks per accept window
  const int lane = (int)(threadIdx.x & 63u);
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // wave index in the workgroup
  __shared__ BmLds32 bm32[1];
  __shared__ DwLds<T> sh;
  if constexpr (sizeof(T) == 4) {
    bm_lds_fill32(bm32[0]);
    __syncthreads();
  }
  const int D = a.D;
  const uint64_t st_end = a.step0 + (uint64_t)a.n_steps;
  const uint64_t blk0 = a.step0 / S;
  // the draw blocks this launch touches: with a.step0 and a.n_steps it fixes
  // the barrier count of every wave (the invariant above)
  const int nblk = a.n_steps > 0 ? (int)((st_end - 1) / S - blk0) + 1 : 0;
  auto opens_window = [](uint64_t b) { return (b & (WB - 1)) == 0; };

  if (wv >= CW) {
    // ---- draw wave ---------------------------------------------------------
    const int dw = wv - CW;
    // block blk of the chain of chain wave w into buffer blk & 1, its window
    // (if `window`) into the window's buffer
    auto fill = [&](int w, uint64_t blk, bool window) __attribute__((always_inline)) {
      const long long c = (long long)blockIdx.x * CW + w;
      if (c >= a.C) return;  // (wave-uniform; no barrier inside)
      const uint32_t cid = a.chain_offset + (uint32_t)c;
      const uint32_t ucid = (uint32_t)__builtin_amdgcn_readfirstlane((int)cid);
      const int buf = (int)(blk & 1u);
      const PhiloxKeys pk = philox_keys(a.seed);
      T z[S];
      momenta_of(draw_block(pk, cid, blk, TAG_MOM, (uint32_t)lane), z, bm32[0]);
#pragma unroll
      for (int k = 0; k < S; ++k) z[k] = (lane < D) ? z[k] : (T)0;
      T kp[S];
#pragma unroll
      for (int k = 0; k < S; ++k) kp[k] = z[k] * z[k];
      group_sum_n_row3(kp);  // totals in row 3
#pragma unroll
      for (int k = 0; k < S; ++k) {
        sh.zs[buf][w][k][lane] = z[k];
        if (lane == 63) sh.kes[buf][w][k] = kp[k] * (T)0.5;
      }
      if (window) sh.lw[(int)((blk / WB) & 1u)][w][lane] = accept_window<T>(a.seed, ucid, blk, lane);
    };
    if (nblk > 0) {
      // a launch's first fill computes its whole window, wherever it starts
      for (int w = dw; w < CW; w += NDW) fill(w, blk0, true);
      __syncthreads();
      for (int i = 0; i < nblk; ++i) {
        if (i + 1 < nblk) {
          const uint64_t nb = blk0 + (uint64_t)i + 1;
          for (int w = dw; w < CW; w += NDW) fill(w, nb, opens_window(nb));
        }
        __syncthreads();
      }
    }
    return;
  }

  // ---- chain wave ------------------------------------------------------------
  // Issue priority over the draw waves, which keep the launch's 0: a draw
  // wave has a whole block's time for its work and takes only the issue
  // cycles the chain waves of its SIMD leave (without it the form is slower
  // than hmc_kernel, profiles/r12).
  __builtin_amdgcn_s_setprio(3);
  const int w = wv;
  const long long c = (long long)blockIdx.x * CW + w;  // wave-uniform
  const bool live = c < a.C;
  const auto tg = tg_.template bind<64, 1>(lane);  // per-lane target view
  T* __restrict__ qs = (T*)a.q;
  const T eps = (T)a.eps;
  const T half = (T)0.5 * eps;
  T q[1], g[1], q1[1], p1[1], g1[1];
  T lp = (T)0;
  q[0] = (T)0;
  g[0] = (T)0;
  if (live) {
    q[0] = (lane < D) ? qs[c * D + lane] : (T)0;
    lp = tg.template eval<64, 1, true>(q, g, lane);
  }
  long long acc = 0;
  const long long Du = (long long)__builtin_amdgcn_readfirstlane(D);
  T* __restrict__ out = (T*)a.samples + (a.sample_row0 * a.C + c) * Du;
  const long long row_stride = a.C * Du;
  uint32_t soff = (uint32_t)(lane * (int)sizeof(T));  // byte offset of this lane's slot in a sample row
  int s = 0;          // transitions done
  uint64_t blk = 0;   // the draw block being run
  T zsA[S], kesA[S], lnuA[S];

  // the transition at position K of block blk (hmc_kernel's step at W1, E = 1,
  // LF = GM_LF_BLOCK; its momentum, kinetic energy and ln u come from zsA,
  // kesA, lnuA)
  auto step = [&](auto kc) __attribute__((always_inline)) {
    constexpr int K = decltype(kc)::v;
    q1[0] = q[0];
    p1[0] = zsA[K];
    g1[0] = g[0];
    const T ke0 = kesA[K];
    T lp1 = lp;
    auto lf = [&]() __attribute__((always_inline)) {
      p1[0] = gfma(g1[0], half, p1[0]);
      q1[0] = gfma(p1[0], eps, q1[0]);
      tg.template eval<64, 1, false>(q1, g1, lane);
      p1[0] = gfma(g1[0], half, p1[0]);
    };
    {
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
    }
    T ke1;
    if (a.L >= 1) {
      p1[0] = gfma(g1[0], half, p1[0]);
      q1[0] = gfma(p1[0], eps, q1[0]);
      using TL = typename Bare<decltype(tg)>::type;
      static_assert(TL::template has_part<64>, "the targets with lf_block reduce logp and the kinetic energy together");
      T sums[2];
      sums[0] = tg.template eval_part<64, 1>(q1, g1, lane);
      p1[0] = gfma(g1[0], half, p1[0]);
      sums[1] = p1[0] * p1[0];
      group_sum_n_row3(sums);
      lp1 = tg.finish(sums[0]);
      ke1 = sums[1] * (T)0.5;
    } else {
      ke1 = group_sum<64>(p1[0] * p1[0]) * (T)0.5;
    }
    // Metropolis accept (NaN log_alpha rejects): the operands are the chain's
    // in row 3 and lane 63's compare decides
    const T log_alpha = (lp1 - lp) + (ke0 - ke1);
    uint32_t hi = (uint32_t)(__builtin_amdgcn_ballot_w64(log_alpha >= lnuA[K]) >> 32);
    asm volatile("" : "+s"(hi));
    if ((hi >> 31) != 0) {
      q[0] = q1[0];
      g[0] = g1[0];
      lp = lp1;
      ++acc;
    }
    if (s >= a.collect_from) {
      asm volatile("" : "+v"(soff));
      if (lane < D) *(T*)((char*)out + soff) = q[0];
      out += row_stride;
    }
  };

  if (nblk > 0) {
    blk = blk0;
    int kb = (int)(a.step0 % S);
    __syncthreads();  // the launch's first block is in buffer blk0 & 1
    for (int i = 0; i < nblk; ++i) {
      if (live) {
        const int buf = (int)(blk & 1u);
        const int wb = (int)((blk / WB) & 1u);
        // the block's momenta (this lane's), and its kinetic energies and
        // ln u at one wave-uniform address each
#pragma unroll
        for (int k = 0; k < S; ++k) {
          zsA[k] = sh.zs[buf][w][k][lane];
          kesA[k] = sh.kes[buf][w][k];
          lnuA[k] = sh.lw[wb][w][(int)(((uint32_t)blk * (uint32_t)S + (uint32_t)k) & 63u)];
        }
        for_each_k<0, S>([&](auto kc) __attribute__((always_inline)) {
          if (decltype(kc)::v >= kb && s < a.n_steps) {
            step(kc);
            ++s;
          }
        });
      }
      kb = 0;
      ++blk;
      __syncthreads();
    }
  }
  if (live) {
    if (lane < D) qs[c * D + lane] = q[0];
    if (lane == 63) {  // lane 63 owns the chain's logp (row 3)
      ((T*)a.logp)[c] = lp;
      a.accepts[c] += acc;
    }
  }
}

}  // namespace gm
