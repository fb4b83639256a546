// gm_plan.cpp — the launch planner (gm_plan.h).
#include "gm_plan.h"

#include <algorithm>

namespace gm {

std::vector<long long> window_ends(WindowSchedule& ws, long long upto, long long sb, long long lim) {
  std::vector<long long> wends;
  for (long long m = 1; m <= upto; ++m) {
    if (m <= sb || !(m < lim)) continue;      // should_collect
    if (m >= ws.next || m + 1 >= lim) {       // note_if_window_end
      ws.next += ws.len;
      ws.len = ws.len * 2 < 400 ? ws.len * 2 : 400;
      wends.push_back(m);
    }
  }
  return wends;
}

std::vector<Segment> plan_segments(const PlanInput& in, const std::vector<long long>& wends) {
  std::vector<Segment> segs;
  if (in.total <= 0 && !in.always_one) return segs;
  size_t wi = 0;
  long long s0 = 0;
  do {
    Segment g;
    g.start = s0;
    long long n = std::max<long long>(0, std::min(in.total - s0, in.chunk));
    if (in.cut_at_warm && s0 < in.warm) n = std::min(n, in.warm - s0);
    const long long first = std::max(s0 + 1, in.sb + 1);  // the first window row from here on
    if (in.slab_rows > 0 && first < in.lim && first <= s0 + n) {
      n = std::min(n, first - 1 - s0 + in.slab_rows);
      n = std::min(n, in.lim - 1 - s0);
    }
    if (wi < wends.size() && wends[wi] <= s0 + n) {  // transition m = s0 + n ends the window
      n = wends[wi] - s0;
      g.update = true;
      ++wi;
    }
    g.n = n;
    const long long hi = std::min(s0 + n, in.lim - 1);
    if (hi >= first) {
      g.first_used = first;
      g.used = hi - first + 1;
    }
    segs.push_back(g);
    s0 += n;
  } while (s0 < in.total);
  if (in.trailing_refind && segs.back().update) {
    Segment g;
    g.start = in.total;
    segs.push_back(g);
  }
  return segs;
}

Plan plan_hmc(long long total, long long chunk, long long warm, bool windows, long long sb, long long eb,
              long long iw, long long slab_rows) {
  Plan p;
  p.lim = warm > eb ? warm - eb : 0;
  WindowSchedule ws(sb, iw);
  std::vector<long long> wends;
  if (windows) wends = window_ends(ws, warm, sb, p.lim);
  p.segs = plan_segments({.total = total, .chunk = chunk, .warm = warm, .cut_at_warm = true, .sb = sb,
                          .lim = windows ? p.lim : 0, .slab_rows = slab_rows}, wends);
  return p;
}

Plan plan_nuts(WindowSchedule& ws, long long total, long long chunk, long long n_discard, bool windows,
               long long sb, long long eb, long long slab_rows) {
  Plan p;
  p.lim = n_discard > eb ? n_discard - eb : 0;
  std::vector<long long> wends;
  if (windows) wends = window_ends(ws, std::min(total, n_discard), sb, p.lim);
  // (without a slab the window rows are the kernel's business: none planned)
  p.segs = plan_segments({.total = total, .chunk = chunk, .sb = sb, .lim = slab_rows > 0 ? p.lim : 0,
                          .slab_rows = slab_rows, .trailing_refind = true, .always_one = true}, wends);
  return p;
}

}  // namespace gm
