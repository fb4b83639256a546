// gm_launch.h — kernel argument blocks (plain structs, device-safe: shared by
// the AOT kernels, the host launchers and the runtime-compiled user-target
// kernels of gm_jit.cpp).
#pragma once
#include <stdint.h>

namespace gm {

// ---- run_progress statistics (gm_track.h, tracker_kernels.hip) -------------
// Per-chain ChainTracker state (stats.rs:24-131), f32 [C][D] and [C]; mean
// is null when tracking is off. n0 = tracker steps before this launch.
struct TrackLaunch {
  float* mean = nullptr;
  float* msq = nullptr;
  float* last = nullptr;
  float* p = nullptr;
  unsigned long long n0 = 0;
};

// ---- per-transition sampler statistics (gm_sampler_set_stats) ---------------
// One record per (transition, chain), [n_transitions][n_chains], written by
// the chain's lane 0 as one aligned store: three values of the sampler dtype
// and a count word, 16 bytes (f32) or 32 (f64; the word's upper half is zero).
// The word, the same for both dtypes:
//   bits 0-23 n_leapfrog (saturating), 24-29 tree_depth, 30 divergent, 31 accepted
template <class T> struct StatsWord;
template <> struct StatsWord<float> { typedef uint32_t type; };
template <> struct StatsWord<double> { typedef uint64_t type; };
template <class T> struct alignas(4 * sizeof(T)) StatsRec {
  T energy;       // the Hamiltonian after the momentum refresh: K(p0) - logp(q)
  T accept_stat;  // NUTS alpha / n_alpha; HMC min(1, exp(log_alpha)), NaN -> 0
  T step_size;    // the step size the transition integrated with
  typename StatsWord<T>::type word;
};
constexpr uint32_t GM_STATS_NLF_MAX = (1u << 24) - 1;
__host__ __device__ constexpr uint32_t stats_word(long long n_leapfrog, int tree_depth, bool divergent,
                                                  bool accepted) {
  return (n_leapfrog > (long long)GM_STATS_NLF_MAX ? GM_STATS_NLF_MAX : (uint32_t)n_leapfrog) |
         ((uint32_t)(tree_depth & 63) << 24) | (divergent ? 1u << 30 : 0u) | (accepted ? 1u << 31 : 0u);
}
// rec is null when statistics are off. Transition s of a launch (0-based) has
// the run index t0 + s and goes to record row t0 + s - first when that is in
// [0, n): `first` is the run's first recorded transition.
struct StatsLaunch {
  void* rec = nullptr;
  long long t0 = 0;
  long long first = 0;
  long long n = 0;
};
// the record of chain c (of C) for transition s of the launch; called by one
// lane of the chain, with st.rec non-null
template <class T>
__device__ __forceinline__ void stats_store(const StatsLaunch& st, long long C, long long c, long long s, T energy,
                                            T accept_stat, T step_size, uint32_t word) {
  const long long r = st.t0 + s - st.first;
  if (r >= 0 && r < st.n) {
    StatsRec<T> v;
    v.energy = energy;
    v.accept_stat = accept_stat;
    v.step_size = step_size;
    v.word = word;
    ((StatsRec<T>*)st.rec)[r * C + c] = v;
  }
}

// ---- HMC -------------------------------------------------------------------
// The long leapfrog loop form of hmc_kernel (hmc_device.h): count-down trips
// of GM_LF_LONG straight-line leapfrogs. The value is also the form's
// lf_unroll / gm_sampler_set_unroll number.
constexpr int GM_LF_LONG = 7;
// The block form: (L - 1) % GM_LF_BLOCK leapfrogs as a binary ladder of
// straight-line pieces, then (L - 1) / GM_LF_BLOCK count-down passes of
// GM_LF_BLOCK straight-line leapfrogs (L = 50: one pass, no ladder). Compiled for one chain per wave at one element per lane and the
// targets with `lf_block` (hmc_block_part.inc); every other kernel runs the
// number as GM_LF_LONG, or as 1 where that is not compiled in either.
constexpr int GM_LF_BLOCK = 49;
// The draw-wave form of the block form (hmc_dw_device.h): the draw waves
// beside the 4 chain waves of a workgroup, and the draw_waves /
// gm_sampler_set_draw_waves number of the form. 1: one draw wave fills for
// the four chains in turn (-3.5 % at the headline; 2: -2.7 %, 4: -0.6 %,
// profiles/r12).
#ifndef GM_DW_WAVES
#define GM_DW_WAVES 1  // (measurement builds: 1, 2 or 4)
#endif

struct HmcLaunch {
  void* q = nullptr;            // [C*D] state, in/out
  void* logp = nullptr;         // [C] out
  long long* accepts = nullptr; // [C] in/out (+= accepted count)
  void* samples = nullptr;      // [rows][C][D]
  long long C = 0;
  int D = 0;
  double eps = 0;
  int L = 0;
  uint64_t seed = 0;
  uint64_t step0 = 0;           // global transition index of the first step
  uint32_t chain_offset = 0;
  int n_steps = 0;
  int collect_from = 0;         // steps s >= collect_from are stored ...
  long long sample_row0 = 0;    // ... at row sample_row0 + (s - collect_from)
  int lf_unroll = 1;            // leapfrog loop form (1, 2, 4, GM_LF_LONG or GM_LF_BLOCK; same results)
  int draw_waves = 0;           // draw waves per workgroup (hmc_dw_device.h; 0: hmc_kernel; same results)
  void* zs = nullptr;          // wide layouts: momentum block scratch [C][S][lanes*elems]
};

// ---- HMC with per-chain step sizes and a diagonal metric --------------------
// (hmc_adapt_device.h). A launch is wholly frozen (MODE 0) or wholly warm-up
// (MODE 1 step size, MODE 2 step size + Welford statistics): the host cuts
// launches at the warm-up's end and at every window end.
struct HmcAdaptLaunch {
  HmcLaunch h;                  // as for the plain kernel (h.eps and h.zs unused)
  void* eps = nullptr;          // [C] per-chain step size, in/out while adapting
  void* eps_bar = nullptr;      // [C] in/out (MODE >= 1)
  void* h_bar = nullptr;        // [C] in/out (MODE >= 1)
  const void* mu = nullptr;     // [C]
  const void* dinv = nullptr;   // [C][D] M^-1
  const void* dsq = nullptr;    // [C][D] sqrt(M) = 1/sqrt(dinv)
  void* rmean = nullptr;        // [C][D] Welford mean, in/out (MODE 2)
  void* rm2 = nullptr;          // [C][D] Welford sum of squared deviations, in/out (MODE 2)
  double delta = 0.8;           // target acceptance
  long long k0 = 0;             // dual-averaging restart counter before this launch
  long long rn0 = 0;            // Welford count before this launch
  long long m0 = 0;             // warm-up transitions before this launch (m = m0 + s + 1)
  long long sb = 0, lim = 0;    // Welford collects while sb < m < lim (lim = n_discard - end_buffer)
  StatsLaunch stats;            // per-transition records (off when stats.rec is null)
};

// ---- HMC with per-chain step sizes and one dense metric for all chains --------
// (hmc_dense_device.h). A launch is wholly frozen (MODE 0) or wholly warm-up
// (MODE 1: step-size dual averaging); the pooled statistics are taken from
// the positions a warm-up launch stores through h.samples.
struct HmcDenseLaunch {
  HmcLaunch h;                  // as for the plain kernel (h.eps and h.zs unused)
  void* eps = nullptr;          // [C] per-chain step size, in/out while adapting
  void* eps_bar = nullptr;      // [C] in/out (MODE 1)
  void* h_bar = nullptr;        // [C] in/out (MODE 1)
  const void* mu = nullptr;     // [C]
  const void* minv = nullptr;   // [D][D] M^-1 = Sigma (symmetric), sampler dtype
  const void* at = nullptr;     // [D][D] at[j*D + i] = A_ij, A = L^-T upper triangular (zeros below)
  double delta = 0.8;           // target acceptance
  long long k0 = 0;             // dual-averaging restart counter before this launch
  StatsLaunch stats;            // per-transition records (off when stats.rec is null)
};
// hmc_dense_kernel's workgroup stays within 64 KiB of LDS: its static part
// (the f32 Box-Muller tables, 3 KiB; the f64 kernels do not use them and the
// compiler drops them there, but one rule serves both dtypes) plus at most
// HMC_DENSE_LDS_DYN bytes of dynamic LDS (target staging, Sigma, slots).
constexpr int HMC_DENSE_LDS_STATIC = 3072;
constexpr int HMC_DENSE_LDS_DYN = 64 * 1024 - HMC_DENSE_LDS_STATIC;
// A user target runs the kernel one chain per lane, layout (1, D): its dynamic
// LDS is Sigma [D][D] and one slot [D] per thread. The block is the largest of
// 256, 128, 64, 32 threads that fits (D <= 64: 32 threads always do).
constexpr unsigned long long hmc_dense_lds_user(int D, int block, int esz) {
  return ((unsigned long long)D * D + (unsigned long long)block * D) * esz;
}
constexpr unsigned hmc_dense_user_block(int D, int esz) {
  return hmc_dense_lds_user(D, 256, esz) <= HMC_DENSE_LDS_DYN   ? 256u
         : hmc_dense_lds_user(D, 128, esz) <= HMC_DENSE_LDS_DYN ? 128u
         : hmc_dense_lds_user(D, 64, esz) <= HMC_DENSE_LDS_DYN  ? 64u
                                                                : 32u;
}

// ---- MH --------------------------------------------------------------------
struct MhLaunch {
  void* q = nullptr;
  void* logp = nullptr;
  long long* accepts = nullptr;
  void* samples = nullptr;
  long long C = 0;
  int D = 0;
  double prop_std = 1;
  uint64_t seed = 0;
  uint64_t step0 = 0;
  uint32_t chain_offset = 0;
  int n_steps = 0;
  int collect_from = 0;
  long long sample_row0 = 0;
  TrackLaunch trk;              // run_progress chain trackers (off when trk.mean is null)
};

// ---- MH with a per-chain proposal scale and a per-chain diagonal shape -------
// (mh_adapt_device.h). A launch is wholly frozen (MODE 0) or wholly warm-up
// (MODE 1 scale, MODE 2 scale + Welford statistics): the host cuts launches at
// the warm-up's end and at every window end, as for HmcAdaptLaunch.
struct MhAdaptLaunch {
  MhLaunch m;                   // as for the plain kernel (m.prop_std unused)
  void* scale = nullptr;        // [C] per-chain proposal scale, in/out while adapting
  void* scale_bar = nullptr;    // [C] in/out (MODE >= 1)
  void* h_bar = nullptr;        // [C] in/out (MODE >= 1)
  const void* mu = nullptr;     // [C]
  const void* diag = nullptr;   // [C][D] proposal shape, or null: all ones
  void* rmean = nullptr;        // [C][D] Welford mean, in/out (MODE 2)
  void* rm2 = nullptr;          // [C][D] Welford sum of squared deviations, in/out (MODE 2)
  double delta = 0.234;         // target acceptance
  long long k0 = 0;             // dual-averaging restart counter before this launch
  long long rn0 = 0;            // Welford count before this launch
  long long m0 = 0;             // warm-up transitions before this launch (m = m0 + s + 1)
  long long sb = 0, lim = 0;    // Welford collects while sb < m < lim (lim = n_discard - end_buffer)
};

// ---- NUTS ------------------------------------------------------------------
// bytes of one HBM subtree-stack entry: three D-vectors, alpha, n, n_alpha,
// padded to whole 128-byte cache lines
inline long long nuts_stack_entry_bytes(int D, int tsz) {
  const long long b = 3LL * D * tsz + tsz + 8;
  return (b + 127) / 128 * 128;
}

struct NutsLaunch {
  void* q = nullptr;
  long long* accepts = nullptr;
  long long* n_leapfrog = nullptr;
  void* samples = nullptr;
  void* eps = nullptr;
  void* eps_bar = nullptr;
  void* h_bar = nullptr;
  void* mu = nullptr;
  void* stk_vec = nullptr;   // HBM stack levels: [C][max_depth] entries of stk_es bytes (gm_nuts.h)
  long long stk_es = 0;
  long long C = 0;
  int D = 0;
  int max_depth = 10;
  double target_accept = 0.8;
  uint64_t seed = 0;
  uint64_t step0 = 0;        // global transition index of this launch's first step
  uint64_t init_step = 0;    // transition counter value used for the init draw
  uint32_t chain_offset = 0;
  int n_steps = 0;
  long long m0 = 0;          // adaptation counter before this launch's first step
  long long n_discard = 0;
  int do_init = 0;           // run init_chain_state first (generic_nuts.rs:731-753)
  long long t0 = 0;          // transitions already done in this run before this launch
  long long row_shift = 0;   // state after t transitions goes to row t - row_shift
  long long n_rows = 0;
  TrackLaunch trk;           // run_progress chain trackers (off when trk.mean is null)
  // mass-matrix warm-up (generic_nuts.rs:33-359); mass_mode 0 = identity, off
  int mass_mode = 0;         // 1 diagonal, 2 dense
  int* mkind = nullptr;      // [C] current metric of each chain: 0 identity, 1 diag, 2 dense
  void* dinv = nullptr;      // [C][D]
  void* dsq = nullptr;       // [C][D]
  void* minv = nullptr;      // [C][D][D]
  void* mchol = nullptr;     // [C][D][D]
  void* mchol_rm = nullptr;  // [C][D][D] + D slack: L row-major (mchol is the per-chain transpose)
  int* rn = nullptr;         // [C] RunningCov::n
  void* rmean = nullptr;     // [C][D]
  void* rm2d = nullptr;      // [C][D]
  void* rm2 = nullptr;       // [C][D][D] (upper triangle used)
  int* updated = nullptr;    // [C] metric replaced at the previous launch's last step
  // levels k < lds_levels of the subtree stack live in LDS (after the
  // target's staging area, at byte offset lds_stack_off), the rest in HBM
  int lds_levels = 0;
  unsigned lds_stack_off = 0;
  // dense metric (mass_mode 2): each chain's M^-1 copied into LDS at kernel
  // start as its packed lower triangle (layout 16 x 2, at byte offset
  // minv_lds_off) when minv_lds, instead of re-read from L2/MALL at every
  // product (nuts_size_lds decides; nuts_device.h minv_packed_lds)
  int minv_lds = 0;
  unsigned minv_lds_off = 0;
  // and its Cholesky factor (the momentum draws), packed the same way, when
  // chol_lds (after M^-1, before the stack levels)
  int chol_lds = 0;
  unsigned chol_lds_off = 0;
  long long sb = 0, eb = 0;  // start_buffer, end_buffer (should_collect, :153-162)
  int do_refind = 0;         // re-find eps for updated chains first (:905-918)
  uint64_t refind_step = 0;  // transition index of the update (probe draws)
  // every chain's metric dense and no warm-up window in this launch: the
  // frozen-dense instantiation (nuts_device.h MASS 3, GM_FROZEN_WAVES waves
  // per SIMD) instead of the general adaptive one
  int dense_frozen = 0;
  // the launch's transition momenta as standard normals [n_steps][C][D]
  // (nuts_momenta_kernel: the same Philox/Box-Muller values the kernel would
  // draw), or null: drawn in the kernel
  const void* zmom = nullptr;
  // with zmom, each transition's start record from the same pass
  // (nuts_starts_kernel, [n_steps][C] of NutsStartRec<T>): the stream key K
  // of the TAG_NUTS_EXP block, ln of its Exp1 uniform, and the doublings'
  // direction bits (bit j: u(K, 2j) < 1/2) -- the values the kernel would
  // compute
  const void* zrec = nullptr;
  // frozen-dense launches (MASS 3) with zmom: the pass has also applied the
  // metric (nuts_dense_momenta_kernel), so zmom holds the momenta p0 = L z
  // themselves and pv0 their M^-1 p0, [n_steps][C][D] each -- the products
  // sample_momentum and the start's kinetic energy would otherwise take in
  // the tree kernel, with the same sums in the same order. Null: the kernel
  // applies L and M^-1 to zmom's normals itself.
  const void* pv0 = nullptr;
};
// The argument block of the recording instantiations (nuts_kernel REC): the
// same block with the records' after it. The others keep NutsLaunch as it
// is: 32 more bytes of kernel arguments changed the frozen-dense kernel's
// register allocation (cfg3_dense about 1 % slower with statistics off).
struct NutsRecLaunch : NutsLaunch {
  StatsLaunch stats;
};
template <bool REC> struct NutsLaunchOf { typedef NutsLaunch type; };
template <> struct NutsLaunchOf<true> { typedef NutsRecLaunch type; };
// the frozen-dense kernel takes its momenta from the pass (pv0 always set;
// nuts_run launches it for no other launch). 0: A/B builds only, the kernel
// applies the metric itself when pv0 is null
#ifndef GM_DENSE_PREP
#define GM_DENSE_PREP 1
#endif
// one start record: 16 bytes (f32) or 32 (f64), read as one 16-byte load
// (key, ln u) and, in f64, one 4-byte load (the direction bits)
template <class T> struct alignas(16) NutsStartRec {
  uint64_t key;
  T lnu;
  uint32_t dir;
};

// waves per SIMD of the NUTS dense-metric instantiations (their launch
// bounds, which the LDS plan of nuts_size_lds follows): the adaptive one
// (MASS 2) at 512 registers, the frozen one (MASS 3)
#ifndef GM_DENSE_WAVES
#define GM_DENSE_WAVES 1
#endif
#ifndef GM_FROZEN_WAVES
#define GM_FROZEN_WAVES 2
#endif
// waves per SIMD of the wide NUTS layouts (one chain per workgroup of
// lanes/64 waves, nuts_wide.hip): 2 up to 16 bytes of state per lane and
// vector (f64 x 2, f32 x 4), else 1 (f64 x 4 spills 58-140 registers at 2)
__host__ __device__ constexpr int nuts_wide_waves(int esz, int E) { return esz * E <= 16 ? 2 : 1; }

}  // namespace gm
