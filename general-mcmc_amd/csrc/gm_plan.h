// gm_plan.h — how a run of transitions is cut into kernel launches: integer
// arithmetic only, no HIP (a host compiler builds gm_plan.cpp alone;
// tools/plan_dump.cpp, tests/test_launch_plan.py). The HMC/MH driver
// (gmcmc_run.cpp) and the NUTS driver (nuts_kernels.hip) launch what
// plan_hmc / plan_nuts return, segment after segment.
#pragma once
#include <cstddef>
#include <vector>

namespace gm {

// The warm-up's metric-window schedule (MassMatrixWarmup, generic_nuts.rs:
// 141-151): a window ends at the first collected transition m >= next, or at
// the last one before lim; the next window is twice as long, up to 400.
struct WindowSchedule {
  long long next = 0, len = 0;
  WindowSchedule() = default;
  WindowSchedule(long long start_buffer, long long initial_window)
      : next((start_buffer > 1 ? start_buffer : 1) + (initial_window > 10 ? initial_window : 10)),
        len(initial_window > 10 ? initial_window : 10) {}
};
// The window ends among transitions m = 1 .. upto (1-based within the run)
// with sb < m < lim; advances ws past them. NUTS passes its persistent state,
// HMC a fresh one per run.
std::vector<long long> window_ends(WindowSchedule& ws, long long upto, long long sb, long long lim);

// One kernel launch: transitions start + 1 .. start + n of the run. update:
// a window ends at its last transition. Of its transitions, `used` are window
// rows (sb < m < lim), the first of them m = first_used.
struct Segment {
  long long start = 0, n = 0;
  bool update = false;
  long long first_used = 0, used = 0;
};

struct PlanInput {
  long long total = 0, chunk = 1;
  long long warm = 0;         // with cut_at_warm: no segment straddles transition `warm`
  bool cut_at_warm = false;
  long long sb = 0, lim = 0;  // the window rows are the m with sb < m < lim (lim 0: none)
  long long slab_rows = 0;    // > 0: a segment holds at most that many window rows, and nothing after the last one
  bool trailing_refind = false;  // an update on the last transition is followed by a segment of length 0
  bool always_one = false;       // total <= 0 still yields one segment
};
// Cuts in this order: chunk, warm-up end, slab, window end.
std::vector<Segment> plan_segments(const PlanInput& in, const std::vector<long long>& wends);

// The rows a segment stores: transitions from s = cf (0-based within the
// segment) on, the first of them at row row0.
struct Collect {
  long long cf, row0;
};
// ... into the sample buffer, whose row 0 is transition collect_from of the run
inline Collect seg_collect(const Segment& g, long long collect_from) {
  long long cf = collect_from - g.start;
  if (cf < 0) cf = 0;
  if (cf > g.n) cf = g.n;
  const long long row0 = g.start - collect_from;
  return {cf, row0 < 0 ? 0 : row0};
}
// ... into the slab: its window rows, from row 0
inline Collect seg_slab(const Segment& g) { return {g.used > 0 ? g.first_used - 1 - g.start : g.n, 0}; }

// The pooled metric's scratch: the slab of window rows [rows][C][D] is bounded
// by GM_DENSE_SLAB_BYTES, the Gram partials of a batch of rows by
// GM_GRAM_PART_BYTES (part_row_bytes: those of one row). At least one row.
constexpr size_t GM_DENSE_SLAB_BYTES = (size_t)64 << 20;
constexpr size_t GM_GRAM_PART_BYTES = (size_t)16 << 20;
inline long long slab_rows_for(long long C, int D, size_t esz) {
  const long long rows = (long long)(GM_DENSE_SLAB_BYTES / ((size_t)C * D * esz));
  return rows > 1 ? rows : 1;
}
inline long long gram_rows_for(size_t part_row_bytes) {
  const long long rows = (long long)(GM_GRAM_PART_BYTES / part_row_bytes);
  return rows > 1 ? rows : 1;
}

// The plans of the two drivers. lim: the first transition past the windows.
struct Plan {
  std::vector<Segment> segs;
  long long lim = 0;
};
// HMC / MH: the first `warm` transitions are the warm-up (0: none), cut at its
// end; windows: it has metric windows (sb, eb, iw); slab_rows: the dense
// metric's slab (0: none).
Plan plan_hmc(long long total, long long chunk, long long warm, bool windows, long long sb, long long eb,
              long long iw, long long slab_rows);
// NUTS: always launches, segments may straddle the warm-up's end; windows:
// a metric is adapted (not in step mode); slab_rows: the pooled metric's slab.
Plan plan_nuts(WindowSchedule& ws, long long total, long long chunk, long long n_discard, bool windows,
               long long sb, long long eb, long long slab_rows);

}  // namespace gm
