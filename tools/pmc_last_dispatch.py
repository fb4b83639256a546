"""Counters of the LAST dispatch of a kernel in a rocprofv3 --pmc run (csv
output), summed over the rows of that dispatch, as one JSON object. With
tools/sweep_hmc.py --rounds 1 as the profiled command the last hmc_kernel
dispatch is the timed launch of --steps transitions.

    python tools/pmc_last_dispatch.py DIR [--kernel hmc_kernel] [--transitions 100]
"""
import argparse
import collections
import csv
import glob
import json
import os

ap = argparse.ArgumentParser()
ap.add_argument("dir")
ap.add_argument("--kernel", default="hmc_kernel")
ap.add_argument("--transitions", type=int, default=0)
a = ap.parse_args()
rows = []
for f in sorted(glob.glob(os.path.join(a.dir, "**", "*counter_collection.csv"), recursive=True)):
    rows += [r for r in csv.DictReader(open(f)) if a.kernel in r["Kernel_Name"]]
if not rows:
    raise SystemExit(f"no {a.kernel} dispatch under {a.dir}")
last = max(int(r["Dispatch_Id"]) for r in rows)
acc = collections.defaultdict(float)
for r in rows:
    if int(r["Dispatch_Id"]) == last:
        acc[r["Counter_Name"]] += float(r["Counter_Value"])
        name = r["Kernel_Name"]
out = {"kernel": name, "dispatch": last, **acc}
waves = acc.get("SQ_WAVES", 0.0)
if waves and a.transitions:
    for c in ("SQ_INSTS_VALU", "SQ_INSTS_SALU"):
        if c in acc:
            out[c.lower().replace("sq_insts_", "") + "_per_wave_transition"] = acc[c] / waves / a.transitions
if acc.get("SQ_WAVE_CYCLES"):
    for c, k in (("SQ_ACTIVE_INST_VALU", "wave_valu_active_frac"), ("SQ_WAIT_ANY", "wave_wait_frac"),
                 ("SQ_WAIT_INST_ANY", "wave_issue_stall_frac")):
        if c in acc:
            out[k] = acc[c] / acc["SQ_WAVE_CYCLES"]
print(json.dumps(out, indent=1))
