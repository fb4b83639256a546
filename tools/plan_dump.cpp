// plan_dump — prints the launch plans of csrc/gm_plan.cpp for the cases on
// standard input (tests/test_launch_plan.py builds it with the host compiler,
// sanitized, and runs it directly). One case per line:
//   hmc <plain|adapt1|adapt2|dense> total chunk collect_from warm sb eb iw slab_rows
//   nuts total chunk n_discard windows sb eb sched_next sched_len slab_rows
// Per segment a line "seg start n cf row0 warm update first_used used" (cf,
// row0 as the HMC driver derives them; 0 for NUTS), then "end sched_next
// sched_len launches".
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "../general-mcmc_amd/csrc/gm_plan.h"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream is(line);
    std::string kind;
    if (!(is >> kind)) continue;
    gm::Plan p;
    gm::WindowSchedule ws;
    if (kind == "hmc") {
      std::string var;
      long long total, chunk, cfrom, warm, sb, eb, iw, slab;
      if (!(is >> var >> total >> chunk >> cfrom >> warm >> sb >> eb >> iw >> slab)) return 2;
      const bool dense = var == "dense";
      if (var == "plain") warm = 0;
      p = gm::plan_hmc(total, chunk, warm, dense || var == "adapt2", sb, eb, iw, dense ? slab : 0);
      for (const gm::Segment& g : p.segs) {
        const bool in_warm = g.start < warm;
        const gm::Collect c = dense && in_warm ? gm::seg_slab(g) : gm::seg_collect(g, cfrom);
        std::printf("seg %lld %lld %lld %lld %d %d %lld %lld\n", g.start, g.n, c.cf, c.row0, (int)in_warm,
                    (int)g.update, g.first_used, g.used);
      }
    } else if (kind == "nuts") {
      long long total, chunk, nd, windows, sb, eb, slab;
      if (!(is >> total >> chunk >> nd >> windows >> sb >> eb >> ws.next >> ws.len >> slab)) return 2;
      p = gm::plan_nuts(ws, total, chunk, nd, windows != 0, sb, eb, slab);
      for (const gm::Segment& g : p.segs)
        std::printf("seg %lld %lld 0 0 0 %d %lld %lld\n", g.start, g.n, (int)g.update, g.first_used, g.used);
    } else {
      return 2;
    }
    std::printf("end %lld %lld %lld\n", ws.next, ws.len, (long long)p.segs.size());
  }
  return 0;
}
