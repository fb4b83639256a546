// gmcmc_run.cpp — the run drivers behind gm_run*, gm_step and the progress
// runs (gmcmc_api.cpp): a run of transitions is cut into kernel launches by
// the planner (gm_plan.h) and enqueued launch after launch. HMC and MH go
// through run_steps' one loop here, NUTS through nuts_run (nuts_kernels.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "gm_sampler.h"

using namespace gm;

// Leapfrog-loop unroll of the HMC kernel (identical results). Measured
// (tools/probe_hmc_scaling.py): x4 is ~12% faster while the grid has at most
// one wave per SIMD (latency bound), and 10-20% slower from two waves per
// SIMD up.
constexpr long long GM_LF_BLOCK_MIN_L1 = 2 * GM_LF_LONG;
static int device_simds() {
  static const int simds = [] {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      cus = 256;
    return 4 * cus;
  }();
  return simds;
}
static int hmc_lf_unroll(long long waves, long long L, bool has_long, bool has_block) {
  const int simds = device_simds();
  // x4 at <= 1 wave per SIMD, x2 at <= 4 (the cfg2 headline), x1 above
  // (cfg4's 8 and the north star's 16 waves per SIMD), measured per regime
  const int form = waves <= simds ? 4 : waves <= 4 * simds ? 2 : 1;
  // The long count-down form (GM_LF_LONG leapfrogs per trip) where x2 ran:
  // above one and up to four waves per SIMD, in the kernels that compile it
  // in (has_long), from the L at which its hot trips carry most of the steps.
  if (form == 2 && has_long && L - 1 >= 2 * GM_LF_LONG) {
    // The block form (passes of GM_LF_BLOCK straight-line leapfrogs) where
    // the kernel has it, from the L at which it measured no slower than the
    // long form (GM_LF_BLOCK_MIN_L1: L = 20 is 1.7 % faster, profiles/r11).
    if (has_block && L - 1 >= GM_LF_BLOCK_MIN_L1) return GM_LF_BLOCK;
    return GM_LF_LONG;
  }
  return form;
}

// The draw-wave form of the block form (hmc_dw_device.h, identical results):
// GM_DW_WAVES draw waves per workgroup where the launch runs the block form in
// the regime in which the form measured faster (profiles/r12): f32, above
// two and a half and up to four chain waves per SIMD (3000 and 4096 chains:
// -3.5 %; 2048 and 1029: +2 %), and a leapfrog loop of at most one pass
// (L = 15 to 50: -3.5 to -5 %; L = 99: +4.7 %). Elsewhere off.
static int hmc_draw_waves(long long waves, long long L, int lf_unroll, bool has_block, bool f32) {
  const int simds = device_simds();
  return has_block && f32 && lf_unroll == GM_LF_BLOCK && L - 1 <= GM_LF_BLOCK && 2 * waves > 5 * simds &&
                 waves <= 4 * simds
             ? GM_DW_WAVES
             : 0;
}

// hipSetDevice only when the calling thread is on another device (the call
// is on every run's path). The current device is asked of the runtime
// (a thread-local read in HIP), never cached here: gm_set_device and the
// other entry points switch devices too.
static hipError_t use_device(int dev) {
  int cur = -1;
  const hipError_t g = hipGetDevice(&cur);
  if (g == hipSuccess && cur == dev) return hipSuccess;
  return hipSetDevice(dev);
}

// One event pair per run (before the first launch, after the last): the
// device time of the run's launches, read back after the run's stream
// synchronize.
static int ensure_run_events(gm_sampler* s) {
  while (s->evs.size() < 2) {
    hipEvent_t ev;
    GM_HIP(hipEventCreate(&ev));
    s->evs.push_back(ev);
  }
  return GM_OK;
}

// ---- per-transition sampler statistics (StatsRun) ---------------------------
int stats_begin(gm_sampler* s, long long total, long long fc, long long first_row) {
  StatsRun& t = s->st;
  t.active = false;
  t.valid = false;
  if (t.mode == 0) return GM_OK;
  if (fc > total) fc = total;
  const long long first = t.mode == 2 ? 0 : fc;
  const long long n = total - first;
  int rc = ensure_buf(&t.buf, &t.cap, (size_t)n * (size_t)s->C * 4 * s->esz);
  if (!rc && s->kind == K_HMC && !s->ha.has) rc = hmc_adapt_ensure(s, t.ident);
  if (rc) return rc;
  t.base = 0;
  t.first = first;
  t.n = n;
  t.first_collected = fc - first;
  t.first_row = first_row;
  t.valid = true;
  t.active = n > 0;
  return GM_OK;
}
// the launch block of a launch whose first transition is `pos` of the current run_steps call
static StatsLaunch stats_launch(const gm_sampler* s, long long pos) {
  StatsLaunch t;
  if (s->st.active) {
    t.rec = s->st.buf;
    t.t0 = s->st.base + pos;
    t.first = s->st.first;
    t.n = s->st.n;
  }
  return t;
}

// ---- HMC / MH: one loop over the planned segments ---------------------------
// The kernel a run's launches go to. A sampler with per-chain step sizes (or a
// recording run of a plain one: hmc_adapt_kernel's frozen mode with the
// identity state of StatsRun, the same bits) takes P_ADAPT, one with the dense
// metric P_DENSE.
// An MH sampler with per-chain proposal scales (gm_mh_set_*) takes
// P_MH_ADAPT, mh_adapt_kernel.
enum HmcPath { P_MH, P_MH_ADAPT, P_PLAIN, P_ADAPT, P_DENSE };

// the launch fields the MH kernel and every HMC kernel take (MhLaunch,
// HmcLaunch), for segment g storing rows c
template <class A>
static A launch_args(const gm_sampler* s, const Segment& g, Collect c) {
  A a;
  a.q = s->d_q;
  a.logp = s->d_logp;
  a.accepts = s->d_acc;
  a.samples = s->d_samples;
  a.C = s->C;
  a.D = s->D;
  a.seed = s->seed;
  a.step0 = s->step + g.start;
  a.chain_offset = s->chain_offset;
  a.n_steps = (int)g.n;
  a.collect_from = (int)c.cf;
  a.sample_row0 = c.row0;
  return a;
}

static hipError_t launch_mh_seg(const gm_sampler* s, const Segment& g, Collect c, const TrackLaunch* trk,
                                LaunchEvents ev) {
  MhLaunch a = launch_args<MhLaunch>(s, g, c);
  a.prop_std = s->prop_std;
  if (trk) {
    a.trk = *trk;
    a.trk.n0 = trk->n0 + (unsigned long long)g.start;
  }
  return launch_mh(s->dt, s->tg, s->lay, a, s->stream, ev);
}

// Per-chain proposal scales / diagonal shape: a warm-up launch (MODE 1 or 2)
// is followed by mh_adapt_window_kernel at a window's end and by
// scale = scale_bar at the warm-up's end; the rest is frozen (MODE 0). Nothing
// here waits for the device, so asynchronous runs stay asynchronous.
static hipError_t launch_mh_adapt_seg(gm_sampler* s, const Segment& g, Collect c, const TrackLaunch* trk,
                                      long long warm, long long lim, LaunchEvents ev) {
  MhAdapt& h = s->ma;
  const bool in_warm = g.start < warm;
  MhAdaptLaunch a;
  a.m = launch_args<MhLaunch>(s, g, c);
  a.m.prop_std = s->prop_std;
  if (trk) {
    a.m.trk = *trk;
    a.m.trk.n0 = trk->n0 + (unsigned long long)g.start;
  }
  a.scale = h.scale;
  a.scale_bar = h.scale_bar;
  a.h_bar = h.h_bar;
  a.mu = h.mu;
  a.diag = h.diag;
  a.rmean = h.rmean;
  a.rm2 = h.rm2;
  a.delta = h.delta;
  a.k0 = h.k;
  a.rn0 = h.rn;
  a.m0 = g.start;
  a.sb = h.sb;
  a.lim = lim;
  // (the window-end update and the copy below go before the run's stop event)
  LaunchEvents kev = ev;
  if (in_warm) kev.stop = nullptr;
  hipError_t e = launch_mh_adapt(s->dt, s->tg, s->lay, a, in_warm ? h.mode : 0, s->stream, kev);
  if (e != hipSuccess || !in_warm) return e;
  h.k += g.n;
  h.rn += g.used;  // (mode 2: its transitions m with sb < m < lim)
  if (g.update && h.rn >= 5) {  // (fewer than 5 positions: nothing changes, the statistics are kept)
    e = launch_mh_adapt_window(s->dt, s->C, s->D, h.reg, h.jit, h.rn, h.scale, h.scale_bar, h.h_bar, h.mu, h.diag,
                               h.rmean, h.rm2, s->stream);
    h.k = 0;
    h.rn = 0;
  }
  if (e == hipSuccess && g.start + g.n == warm) {  // the warm-up is over: scale = scale_bar, frozen from here on
    h.armed = false;
    e = hipMemcpyAsync(h.scale, h.scale_bar, (size_t)s->C * s->esz, hipMemcpyDeviceToDevice, s->stream);
  }
  if (e == hipSuccess && ev.stop) e = hipEventRecord(ev.stop, s->stream);
  return e;
}

// the warm-up is over: eps = eps_bar, frozen from here on
static hipError_t hmc_warm_end(gm_sampler* s, HmcAdapt& h) {
  h.armed = false;
  return hipMemcpyAsync(h.eps, h.eps_bar, (size_t)s->C * s->esz, hipMemcpyDeviceToDevice, s->stream);
}

// Per-chain step sizes / diagonal metric: a warm-up launch (MODE 1 or 2) is
// followed by hmc_adapt_window_kernel at a window's end and by eps = eps_bar
// at the warm-up's end; the rest is frozen (MODE 0). Nothing here waits for
// the device, so asynchronous runs stay asynchronous.
static hipError_t launch_adapt_seg(gm_sampler* s, HmcAdapt& h, const HmcLaunch& base, const Segment& g, long long warm,
                                   long long lim, LaunchEvents ev) {
  const bool in_warm = g.start < warm;
  HmcAdaptLaunch a;
  a.h = base;
  a.eps = h.eps;
  a.eps_bar = h.eps_bar;
  a.h_bar = h.h_bar;
  a.mu = h.mu;
  a.dinv = h.dinv;
  a.dsq = h.dsq;
  a.rmean = h.rmean;
  a.rm2 = h.rm2;
  a.delta = h.delta;
  a.k0 = h.k;
  a.rn0 = h.rn;
  a.m0 = g.start;
  a.sb = h.sb;
  a.lim = lim;
  a.stats = stats_launch(s, g.start);
  hipError_t e = launch_hmc_adapt(s->dt, s->tg, s->lay, a, in_warm ? h.mode : 0, s->stream, ev);
  if (e != hipSuccess || !in_warm) return e;
  h.k += g.n;
  h.rn += g.used;  // (mode 2: its transitions m with sb < m < lim)
  if (g.update && h.rn >= 5) {  // (fewer than 5 positions: nothing changes, the statistics are kept)
    e = launch_hmc_adapt_window(s->dt, s->C, s->D, h.reg, h.jit, h.rn, h.eps, h.eps_bar, h.h_bar, h.mu, h.dinv,
                                h.dsq, h.rmean, h.rm2, s->stream);
    h.k = 0;
    h.rn = 0;
  }
  if (e == hipSuccess && g.start + g.n == warm) e = hmc_warm_end(s, h);
  return e;
}

// The dense metric: MODE 1 launches during the warm-up. While a window is open
// (sb < m < lim) the launch stores its post-accept positions to the scratch
// slab through the sample-store path (a warm-up launch collects nothing
// else); after it the pooled statistics take the slab's rows on the stream,
// and at a window end hmc_dense_window_kernel replaces the metric. The run's
// stop event goes after all of that. Nothing here waits for the device.
static hipError_t launch_dense_seg(gm_sampler* s, const HmcLaunch& base, const Segment& g, long long warm,
                                   LaunchEvents ev) {
  HmcAdapt& h = s->ha;
  HmcDense& d = s->hd;
  const bool in_warm = g.start < warm;
  HmcDenseLaunch a;
  a.h = base;
  if (in_warm) a.h.samples = d.ps.slab;
  a.eps = h.eps;
  a.eps_bar = h.eps_bar;
  a.h_bar = h.h_bar;
  a.mu = h.mu;
  a.minv = d.minv_t;
  a.at = d.at_t;
  a.delta = h.delta;
  a.k0 = h.k;
  a.stats = stats_launch(s, g.start);
  LaunchEvents kev = ev;
  if (in_warm) kev.stop = nullptr;
  hipError_t e = launch_hmc_dense(s->dt, s->tg, s->lay, a, in_warm ? 1 : 0, s->stream, kev);
  if (e != hipSuccess || !in_warm) return e;
  h.k += g.n;
  if (g.used > 0) e = pooled_accumulate(s->dt, d.ps, g.used, s->C, s->D, &h.rn, d.c0, d.s1, d.S2, s->stream);
  if (e == hipSuccess && g.update && h.rn >= 5) {  // (fewer than 5 rows: nothing changes, the statistics are kept)
    e = launch_hmc_dense_window(s->dt, s->D, s->C, 1, h.rn * s->C, h.reg, h.jit, d.s1, d.S2, d.sig_in, d.minv, d.afac,
                                d.minv_t, d.at_t, d.counters, 1, 1, h.eps, h.eps_bar, h.h_bar, h.mu, s->stream);
    h.k = 0;
    h.rn = 0;
  }
  if (e == hipSuccess && g.start + g.n == warm) e = hmc_warm_end(s, h);
  if (e == hipSuccess && ev.stop) e = hipEventRecord(ev.stop, s->stream);
  return e;
}

int run_steps(gm_sampler* s, long long total, long long collect_from, int progress, const TrackLaunch* trk,
              const StepHook* hook, long long chunk_override) {
  // the n_discard of a gm_run* call, consumed here: gm_step and the
  // collection part of run_progress never start a warm-up
  const long long pending_warm = s->ha.pending_warm;
  s->ha.pending_warm = 0;
  GM_HIP(use_device(s->device));
  s->last_ms = 0;
  s->last_launches = 0;
  s->last_ms_pending = false;
  // NUTS always launches: init_chain_state + row 0 even with zero transitions
  if (total <= 0 && s->kind != K_NUTS) return GM_OK;
  const long long chunk = chunk_override > 0 ? chunk_override : s->steps_per_launch;
  if (s->kind == K_NUTS) {
    const StatsLaunch sl = stats_launch(s, 0);
    return nuts_run(s->nuts, s->dt, s->tg, s->lay, s->d_q, s->d_acc, s->d_samples, s->C, s->D, s->target_accept,
                    s->seed, &s->step, s->chain_offset, total, collect_from, progress, chunk, s->stream, s->evs,
                    &s->last_ms, &s->last_launches, trk, hook, sl.rec ? &sl : nullptr);
  }
  int rc = ensure_run_events(s);
  if (rc) return rc;
  // (the long form is compiled into the plain kernel's one-chain-per-wave
  // layouts with at most two elements per lane, hmc_part.inc, and the warm-up
  // and dense-metric kernels run it as x1; chosen at one element per lane
  // only: at two, 4096 chains x 128-D, it measured 3.5 % slower than x2,
  // profiles/r10/ab_hmc_64x2_4096.log)
  const bool adapt_path = s->ha.has || s->st.active;
  const bool has_long = !adapt_path && s->lay.lanes == 64 && s->lay.elems == 1;
  // (the block form: hmc_part.inc, the targets with lf_block)
  const bool has_block = has_long && s->tg.kind == GM_TARGET_ROSENBROCK;
  const long long waves = (s->C * s->lay.lanes + 63) / 64;
  // (a forced draw-wave count takes the block form with it where the loop
  // form is left to the rule: the draw-wave form is compiled for that one)
  const bool dw_forced = s->kind == K_HMC && has_block && s->draw_waves == GM_DW_WAVES;
  const int lf_unroll = s->kind != K_HMC ? 1 : s->lf_unroll ? s->lf_unroll
                        : dw_forced      ? GM_LF_BLOCK
                                         : hmc_lf_unroll(waves, s->L, has_long, has_block);
  s->last_unroll = lf_unroll;
  // the draw waves of this run's launches: the rule, or the forced count where
  // the form is compiled (the block form's kernels at GM_DW_WAVES), else off
  const int draw_waves = s->kind != K_HMC || !has_block || lf_unroll != GM_LF_BLOCK ? 0
                         : s->draw_waves < 0 ? hmc_draw_waves(waves, s->L, lf_unroll, has_block, s->dt == GM_F32)
                         : s->draw_waves == GM_DW_WAVES ? GM_DW_WAVES
                                                        : 0;
  s->last_draw_waves = draw_waves;
  const HmcPath path = s->kind != K_HMC ? (s->ma.has ? P_MH_ADAPT : P_MH)
                       : !adapt_path     ? P_PLAIN
                       : s->hd.on        ? P_DENSE
                                         : P_ADAPT;
  // The first `warm` transitions are the warm-up, cut at every metric window's
  // end (diagonal: mode 2) and at its own end.
  HmcAdapt& h = s->ha.has ? s->ha : s->st.ident;
  const MhAdapt& mh = s->ma;
  const long long warm = path >= P_ADAPT && s->ha.armed && s->ha.mode ? std::min(pending_warm, total)
                         : path == P_MH_ADAPT && mh.armed && mh.mode  ? std::min(pending_warm, total)
                                                                      : 0;
  const long long slab_rows = path == P_DENSE ? slab_rows_for(s->C, s->D, s->esz) : 0;
  const Plan plan = path == P_MH_ADAPT
                        ? plan_hmc(total, chunk, warm, mh.mode == 2, mh.sb, mh.eb, mh.iw, 0)
                        : plan_hmc(total, chunk, warm, path == P_DENSE || (path == P_ADAPT && h.mode == 2), h.sb, h.eb,
                                   h.iw, slab_rows);
  // scratch once, before anything is enqueued
  if (path == P_DENSE && warm > 0 && plan.lim - 1 > h.sb)
    rc = pooled_scratch_ensure(s->hd.ps, std::min(std::min(slab_rows, chunk), plan.lim - 1 - h.sb), s->C, s->D,
                               s->esz);
  if (path == P_PLAIN && layout_is_wide(s->lay))
    rc = ensure_buf(&s->d_zs, &s->zs_bytes,
                    (size_t)s->C * (s->dt == GM_F32 ? 4 : 2) * s->lay.lanes * s->lay.elems * s->esz);
  if (rc) return rc;
  for (const Segment& g : plan.segs) {
    LaunchEvents ev;  // start with the first launch, stop with the last
    if (g.start == 0) ev.start = s->evs[0];
    if (g.start + g.n >= total) ev.stop = s->evs[1];
    const Collect c = path == P_DENSE && g.start < warm ? seg_slab(g) : seg_collect(g, collect_from);
    hipError_t e;
    if (path == P_MH) {
      e = launch_mh_seg(s, g, c, trk, ev);
    } else if (path == P_MH_ADAPT) {
      e = launch_mh_adapt_seg(s, g, c, trk, warm, plan.lim, ev);
    } else {
      HmcLaunch a = launch_args<HmcLaunch>(s, g, c);
      a.eps = s->eps;
      a.L = s->L;
      a.lf_unroll = lf_unroll;
      a.draw_waves = draw_waves;
      if (path == P_PLAIN) {
        if (layout_is_wide(s->lay)) a.zs = s->d_zs;  // the momentum scratch
        e = launch_hmc(s->dt, s->tg, s->lay, a, s->stream, ev);
      } else if (path == P_ADAPT) {
        e = launch_adapt_seg(s, h, a, g, warm, plan.lim, ev);
      } else {
        e = launch_dense_seg(s, a, g, warm, ev);
      }
    }
    if (e != hipSuccess) {
      set_error(std::string("kernel launch failed: ") + hipGetErrorString(e));
      return GM_EHIP;
    }
    if (hook && *hook) {
      rc = (*hook)(g.start + g.n);
      if (rc) return rc;
    }
  }
  s->step += total;
  s->total_steps += total;
  if (!(s->async_runs && s->may_async)) GM_HIP(hipStreamSynchronize(s->stream));
  s->last_ms_pending = true;
  s->last_launches = (long long)plan.segs.size();
  return GM_OK;
}

int run_impl(gm_sampler* s, int64_t n_collect, int64_t n_discard, int progress) {
  GM_REQ(s, "sampler is NULL");
  s->last_rows = n_collect;
  GM_REQ(n_collect >= 0 && n_discard >= 0, "n_collect and n_discard must be >= 0");
  GM_HIP(use_device(s->device));
  int rc = ensure_buf(&s->d_samples, &s->samples_bytes, (size_t)n_collect * s->C * s->D * s->esz);
  if (rc) return rc;
  long long total = n_discard + n_collect;
  s->ha.pending_warm = n_discard;
  s->st.valid = false;
  StatsScope scope{s};
  long long fc = n_discard, first_row = 0;
  if (s->kind == K_NUTS && !progress) {
    // NUTS::run performs n_collect + n_discard - 1 transitions (nuts.rs:232-257);
    // row r is the state after n_discard + r of them.
    if (n_collect == 0) return GM_OK;
    total = n_discard + n_collect - 1;
    // (transition t ends in row t + 1 - n_discard; row 0 of a run without burn-in is the start state)
    fc = n_discard > 0 ? n_discard - 1 : 0;
    first_row = n_discard > 0 ? 0 : 1;
  }
  rc = stats_begin(s, total, fc, first_row);
  if (rc) return rc;
  return run_steps(s, total, n_discard, progress ? 1 : 0);
}
