// gm_nuts.h — host-side interface of the NUTS engine (nuts_kernels.hip).
#pragma once
#include <functional>
#include <vector>

#include "gm_internal.h"
#include "gm_plan.h"

namespace gm {

constexpr int NUTS_DEFAULT_MAX_DEPTH = 10;
constexpr int NUTS_MAX_DEPTH_LIMIT = 30;

struct NutsState {
  bool inited = false;
  int max_depth = 0;
  void* eps = nullptr;      // [C] T   step size (generic_nuts.rs:573)
  void* eps_bar = nullptr;  // [C] T   (:581)
  void* h_bar = nullptr;    // [C] T   (:582)
  void* mu = nullptr;       // [C] T   (:580)
  // subtree-stack levels held in HBM: per chain max_depth entries of
  // stk_es bytes, entry = [3][D] T (left-subtree first q, first p, proposal
  // q), then alpha (T), n, n_alpha (int); one contiguous stretch per (chain,
  // level) (nuts_stack_entry_bytes)
  void* stk_vec = nullptr;
  long long stk_es = 0;
  long long lds_levels_cap = -1;  // subtree-stack levels in LDS: -1 as many as fit
  int dense_minv_lds = 1;     // dense M^-1 in LDS: 1 packed (the default: room for 6 stack levels),
                              // 2 full when it fits (else packed), 0 off
  int dense_chol_lds = 0;     // its Cholesky factor too (packed form only)
  int plan[6] = {0, 0, 0, 0, 0, 0};  // last launch: stack levels in LDS, M^-1 form, offset, L form, offset, frozen
  long long* n_leapfrog = nullptr;  // [C] cumulative leapfrog count
  long long m = 0;            // transitions since the last init_chain_state (:735)
  long long n_discard = 0;    // warm-up length of the current run (:734)
  // mass-matrix warm-up (GenericNUTS::new_with_mass_matrix, generic_nuts.rs:33-359)
  int mass_mode = 0;          // 0 off (identity), 1 diagonal, 2 dense
  long long m_sb = 0, m_eb = 0;
  double m_reg = 0, m_jit = 0;
  WindowSchedule sched;       // MassMatrixWarmup window schedule (persists across runs)
  int* mkind = nullptr;       // [C] 0 identity, 1 diagonal, 2 dense
  void* dinv = nullptr;       // [C][D]
  void* dsq = nullptr;        // [C][D]
  void* minv = nullptr;       // [C][D][D]
  void* mchol = nullptr;      // [C][D][D]
  int* rn = nullptr;          // [C] RunningCov
  void* rmean = nullptr;      // [C][D]
  void* rm2d = nullptr;       // [C][D]
  void* rm2 = nullptr;        // [C][D][D]
  int* updated = nullptr;     // [C]
  void* mscratch = nullptr;   // [C][4 + convention][D][D] dense update workspace
  // metric convention (gm_nuts_set_metric_convention): 0 the reference's
  // M = Sigma_hat, 1 whitening M^-1 = Sigma_hat; pooled: one Sigma_hat from
  // all chains' window rows (whitening, 2 <= D <= 64), in float64
  int convention = 0, pooled = 0;
  // allocated while convention == 1 and 2 <= D <= 64:
  double* pool = nullptr;      // Sigma_hat [D][D], chol(Sigma_hat^-1) [D][D] (the masters), sig_in [D][D],
                               // then the open window's c0 [D], s1 [D], S2 [D][D]
  long long* pcount = nullptr; // updates, failed, the open window's rows (set when a checkpoint is written), 0
  int* pok = nullptr;          // the last window kernel's outcome
  void* pcopy = nullptr;       // the masters rounded to the sampler dtype, 2 [D][D]
  long long p_rn = 0;          // rows in the open window's pooled statistics
  PooledScratch ps;            // a warm-up launch's window rows [rows][C][D], Gram partials
  double* p_sig() const { return pool; }
  double* p_lp(int D) const { return pool + (size_t)D * D; }
  double* p_in(int D) const { return pool + 2 * (size_t)D * D; }
  double* p_c0(int D) const { return pool + 3 * (size_t)D * D; }
  double* p_s1(int D) const { return pool + 3 * (size_t)D * D + D; }
  double* p_S2(int D) const { return pool + 3 * (size_t)D * D + 2 * (size_t)D; }
  static size_t pool_doubles(int D) { return 4 * (size_t)D * D + 2 * (size_t)D; }
  void* zbuf = nullptr;       // [steps][C][D] momentum normals of a launch (nuts_momenta_kernel)
  bool momentum_pass = true;  // gm_nuts_set_momentum_pass
#ifndef GM_NUTS_ZBUF_MAX
#define GM_NUTS_ZBUF_MAX (4ull << 30)  // at most 4 GiB (cfg3: 1 GiB per 500-transition launch)
#endif
  size_t zbuf_bytes = 0;
};

int nuts_init_state(NutsState* ns, gm_dtype dt, long long C, int D, int max_depth);
void nuts_free_state(NutsState* ns);
// Called after each launch with the transitions done so far in the run (the
// launch may still be in flight); non-zero aborts the run with that status.
using StepHook = std::function<int(long long)>;
// progress = 0: NUTS::run semantics; 1: run_progress semantics (see gmcmc.h);
// 2: NUTS::step, `total` transitions continuing the state (no init, nothing
// collected, n_discard ignored: the last run's)
int nuts_run(NutsState& ns, gm_dtype dt, const TargetDev& tg, const Layout& lay, void* q,
             long long* accepts, void* samples, long long C, int D, double target_accept,
             uint64_t seed, uint64_t* step, uint32_t chain_offset, long long total,
             long long n_discard, int progress, long long steps_per_launch, hipStream_t st,
             std::vector<hipEvent_t>& evs, double* ms, long long* launches,
             const TrackLaunch* trk = nullptr, const StepHook* hook = nullptr,
             const StatsLaunch* stats = nullptr);  // stats: the run's records; t0 the run index of this call's first transition
int nuts_set_mass(NutsState* ns, gm_dtype dt, long long C, int D, int mode, long long start_buffer,
                  long long end_buffer, long long initial_window, double regularize, double jitter);
int nuts_get_mass(NutsState& ns, gm_dtype dt, long long C, int D, int32_t* kind, void* dinv, void* dsqrt,
                  void* minv, void* mchol);
// the metric convention of the window ends from now on; allocates or frees
// the pooled state; the sampler is unchanged on an error
int nuts_set_convention(NutsState* ns, gm_dtype dt, long long C, int D, int convention, int pooled);
// the float64 masters [D][D] and the counters (any may be null)
int nuts_get_pooled(NutsState& ns, int D, double* sigma, double* chol_prec, long long* updates,
                    long long* failed);
// sigma [D][D] (validated by the caller) as every chain's dense whitening
// metric, factored by the window-end kernel; waits for the stream
int nuts_set_pooled_metric(NutsState& ns, gm_dtype dt, long long C, int D, const double* sigma, hipStream_t st);
int nuts_get_step_size(NutsState& ns, gm_dtype dt, long long C, double* eps, double* eps_bar);
int nuts_get_leapfrogs(NutsState& ns, long long C, long long* out);

}  // namespace gm
