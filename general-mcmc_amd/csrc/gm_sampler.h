// gm_sampler.h — the sampler object behind the C ABI (include/gmcmc.h) and
// what the two translation units that work on it share: gmcmc_api.cpp (entry
// points, setters, state save/load) and gmcmc_run.cpp (the run drivers).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "gm_nuts.h"

#define GM_HIP(expr)                                                                   \
  do {                                                                                 \
    hipError_t _e = (expr);                                                            \
    if (_e != hipSuccess) {                                                            \
      gm::set_error(std::string("HIP error ") + hipGetErrorString(_e) + " at " #expr); \
      return GM_EHIP;                                                                  \
    }                                                                                  \
  } while (0)

#define GM_REQ(cond, msg)   \
  do {                      \
    if (!(cond)) {          \
      gm::set_error(msg);   \
      return GM_EINVAL;     \
    }                       \
  } while (0)

enum SamplerKind { K_HMC = 1, K_MH = 2, K_NUTS = 3 };

// HMC with per-chain step sizes, a diagonal metric and their warm-up
// (gm_hmc_set_*; hmc_adapt_device.h). `has`: the per-chain arrays exist and
// the sampler runs hmc_adapt_kernel instead of hmc_kernel.
struct HmcAdapt {
  bool has = false;
  int mode = 0;        // 0 none, 1 step size, 2 step size + diagonal metric
  bool armed = false;  // the next run's n_discard transitions are the warm-up
  double delta = 0.8;
  long long sb = 0, eb = 0, iw = 0;
  double reg = 0, jit = 0;
  // dual-averaging restart counter and Welford count: the window schedule
  // depends on the transition index only, so they are the same for every chain
  long long k = 0, rn = 0;
  long long pending_warm = 0;  // n_discard of the gm_run* call that is entering run_steps
  void *eps = nullptr, *eps_bar = nullptr, *h_bar = nullptr, *mu = nullptr;       // [C]
  void *dinv = nullptr, *dsq = nullptr, *rmean = nullptr, *rm2 = nullptr;         // [C][D]
};

// MH with a per-chain proposal scale, a per-chain diagonal proposal shape and
// their warm-up (gm_mh_set_*; mh_adapt_device.h). `has`: the per-chain arrays
// [C] exist and the sampler runs mh_adapt_kernel instead of mh_kernel. The
// [C][D] arrays exist only once a shape was set or mode 2 was armed (`has_diag`);
// without them the shape is all ones.
struct MhAdapt {
  bool has = false, has_diag = false;
  int mode = 0;        // 0 none, 1 scale, 2 scale + diagonal shape
  bool armed = false;  // the next run's n_discard transitions are the warm-up
  double delta = 0.234;
  long long sb = 0, eb = 0, iw = 0;
  double reg = 0, jit = 0;
  long long k = 0, rn = 0;  // dual-averaging restart counter and Welford count (the same for every chain)
  void *scale = nullptr, *scale_bar = nullptr, *h_bar = nullptr, *mu = nullptr;  // [C]
  void *diag = nullptr, *rmean = nullptr, *rm2 = nullptr;                        // [C][D]
};

// One dense metric shared by all chains (gm_hmc_set_dense_*;
// hmc_dense_device.h). `on`: the sampler runs hmc_dense_kernel. The per-chain
// step sizes, the dual-averaging state, the window configuration and the
// counters k / rn (here: rows of pooled positions in the open window) are
// HmcAdapt's, which a dense-metric sampler always has.
struct HmcDense {
  bool on = false;
  double *minv = nullptr, *afac = nullptr;            // [D][D] float64 masters: Sigma, A = L^-T (row-major)
  double *c0 = nullptr, *s1 = nullptr, *S2 = nullptr;  // pooled statistics: pivot [D], sums [D], [D][D]
  double* sig_in = nullptr;                            // [D][D] staging of gm_hmc_set_dense_metric
  void *minv_t = nullptr, *at_t = nullptr;             // sampler-dtype copies (at_t[j*D + i] = A_ij)
  long long* counters = nullptr;                       // [2] metric updates, failed factorisations
  gm::PooledScratch ps;                                // warm-up positions of one launch, gram partials
};

// Per-transition sampler statistics (gm_sampler_set_stats; gm_launch.h
// StatsRec). A run option: nothing of it enters a checkpoint.
struct StatsRun {
  int mode = 0;         // 0 off, 1 collected, 2 all
  void* buf = nullptr;  // the last recording run's records [n][C]
  size_t cap = 0;
  bool active = false;  // a gm_run* call is recording (gm_step never does)
  bool valid = false;   // the last run recorded: buf, n, first_collected and first_row are its
  long long base = 0;   // run index of the first transition of the next run_steps call
  long long first = 0;  // the run's first recorded transition
  long long n = 0;      // transitions recorded
  long long first_collected = 0, first_row = 0;
  // a plain HMC sampler's recording launches: per-chain state of the creation
  // step size and the identity metric for hmc_adapt_kernel's frozen mode
  HmcAdapt ident;
  void* scratch = nullptr;  // the reduction's scratch and outputs
  size_t scratch_cap = 0;
};

struct gm_sampler {
  int kind = 0;
  gm_dtype dt = GM_F32;
  size_t esz = 4;
  long long C = 0;
  int D = 0;
  int device = 0;
  hipStream_t stream = nullptr;
  gm::TargetDev tg;
  void* d_mu = nullptr;
  void* d_prec = nullptr;
  double eps = 0;
  int L = 0;
  double prop_std = 1;
  double target_accept = 0.8;
  int max_depth = 10;
  uint64_t seed = 0;
  uint64_t step = 0;
  uint32_t chain_offset = 0;
  void* d_q = nullptr;
  void* d_logp = nullptr;
  long long* d_acc = nullptr;
  void* d_samples = nullptr;
  size_t samples_bytes = 0;
  void* d_tmp = nullptr;
  size_t tmp_bytes = 0;
  void* h_stage[2] = {nullptr, nullptr};  // pinned D2H staging slots (gm_copy_samples)
  hipEvent_t stage_ev[2] = {nullptr, nullptr};
  void* d_zs = nullptr;  // wide-layout HMC momentum scratch
  size_t zs_bytes = 0;
  gm::Layout lay;
  bool lay_from_wide = false;  // NUTS: a wide layout replaced for a dense metric (gm_nuts_set_mass_adaptation)
  gm::Layout lay_wide{};            // ... and that layout
  long long steps_per_launch = 1000;
  int lf_unroll = 0;  // HMC leapfrog-loop form: 0 by the wave count and L (hmc_lf_unroll), else 1, 2, 4, GM_LF_LONG or GM_LF_BLOCK
  int draw_waves = -1;  // HMC draw-wave form (hmc_dw_device.h): -1 by the regime (hmc_draw_waves), 0 off, else the draw waves per workgroup
  int last_draw_waves = 0;  // the draw waves of the last run's launches (gm_sampler_last_draw_waves)
  std::vector<hipEvent_t> evs;
  double last_ms = 0;
  long long last_launches = 0;
  int last_unroll = 0;  // the leapfrog loop form of the last run's launches (gm_sampler_last_unroll)
  bool last_ms_pending = false;  // HMC/MH: last_ms is read from evs[0..1] on request
  bool async_runs = false;       // HMC/MH runs return after enqueueing (gm_sampler_set_async)
  bool may_async = false;        // set by the entry points that honour async_runs
  long long total_steps = 0;  // transitions since creation
  long long last_rows = 0;    // sample rows produced by the last run
  gm::NutsState nuts;
  HmcAdapt ha;
  HmcDense hd;
  MhAdapt ma;
  StatsRun st;
  // run_progress statistics: per-chain trackers (MH, NUTS) and a
  // MultiChainTracker (HMC), one allocation each (TrackSet)
  void* d_trk = nullptr;
  size_t trk_bytes = 0;
  unsigned long long trk_n = 0;  // ChainTracker steps taken (0: no stats yet)
  void* d_mct = nullptr;
  size_t mct_bytes = 0;
};

// Views into one tracker allocation: mean, msq, last [C*D]; p [C]; flags [C]
// (int); rhat [D]; scalar [1].
struct TrackSet {
  float *mean, *msq, *last, *p, *rhat, *scalar;
  int* flags;
  static size_t bytes(long long C, int D) { return sizeof(float) * (3 * (size_t)C * D + 2 * C + D + 1); }
  TrackSet(void* base, long long C, int D) {
    float* f = (float*)base;
    mean = f;
    msq = f + (size_t)C * D;
    last = f + 2 * (size_t)C * D;
    p = f + 3 * (size_t)C * D;
    flags = (int*)(p + C);
    rhat = (float*)(flags + C);
    scalar = rhat + D;
  }
  gm::TrackLaunch launch() const {
    gm::TrackLaunch t;
    t.mean = mean;
    t.msq = msq;
    t.last = last;
    t.p = p;
    return t;
  }
};

// Allocates the per-chain arrays of h in their start state (gmcmc_api.cpp).
int hmc_adapt_ensure(gm_sampler* s, HmcAdapt& h);

// ---- the run drivers (gmcmc_run.cpp) ----------------------------------------
// The start of a recording run of `total` transitions, before anything is
// launched: the record buffer (an allocation failure is a clean error) and,
// for a plain HMC sampler, the identity per-chain state. fc: the first
// transition whose resulting state is a collected row, first_row: that row.
// StatsScope ends the recording when the run's entry point returns.
int stats_begin(gm_sampler* s, long long total, long long fc, long long first_row);
struct StatsScope {
  gm_sampler* s;
  ~StatsScope() { s->st.active = false; }
};
// Runs `total` transitions; transitions with index >= collect_from (0-based
// within this call) are stored at sample rows (index - collect_from).
int run_steps(gm_sampler* s, long long total, long long collect_from, int progress,
              const gm::TrackLaunch* trk = nullptr, const gm::StepHook* hook = nullptr,
              long long chunk_override = 0);
// gm_run / gm_run_device: n_discard transitions, then n_collect sample rows
int run_impl(gm_sampler* s, int64_t n_collect, int64_t n_discard, int progress);
