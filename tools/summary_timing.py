"""Times the device posterior summary on the README's diagnostic shape:
4096 chains x 1000 draws x 64 parameters, f32 device samples of cfg2's sampler
(HMC, 64-D Rosenbrock, step 0.01, L = 50).

    python tools/summary_timing.py                 # the three figures, one JSON line
    python tools/summary_timing.py --only summary  # warm-up + one call (to run under a kernel trace)

Timed, each as the median of --runs calls after one warm-up call, with a host
clock around calls that end in a device synchronisation:
  DeviceSamples.summary()         the device route
  DeviceSamples.split_rhat_ess()  the plain estimator
  to_host() + tests/_rank_diag_ref.summary on --threads host threads

The line also carries the bytes the sort's passes move, computed from the
shape: per element and radix pass the histogram reads the key, the scatter
reads and writes key + index. Kernel shares come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/summary_timing.py --only summary`.
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, runs):
    fn()  # warm-up
    ts = []
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts), ts


def sort_bytes(m: int, params: int, dtype, plan) -> int:
    """Bytes moved by the radix passes of the two sorts (values, then folded values)."""
    if m <= plan["lds_max"]:
        return 0
    kb = np.dtype(dtype).itemsize
    per_elem = 0
    for key in (kb, 8):
        passes = key * 8 // plan["radix_bits"]
        per_elem += passes * (key + 2 * (key + 4))
    return per_elem * m * params


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host-runs", type=int, default=5)
    ap.add_argument("--threads", type=int, default=min(16, len(os.sched_getaffinity(0))))
    ap.add_argument("--only", choices=["summary"], default=None)
    a = ap.parse_args()

    import general_mcmc_amd as gm
    from tests import _rank_diag_ref as ref

    x0 = gm.init_det(a.chains, a.dim, np.float32)
    s = gm.HMC(gm.RosenbrockND(), x0, 0.01, 50).set_seed(42)
    ds = s.run_positions(a.draws, 100)
    if a.only == "summary":
        ds.summary()
        ds.summary()
        print(json.dumps({"only": "summary", "calls": 2}))
        return
    res = {"shape": [a.chains, a.draws, a.dim], "dtype": "float32", "runs": a.runs}
    res["summary_s"], res["summary_all_s"] = timed(ds.summary, a.runs)
    res["split_rhat_ess_s"], _ = timed(ds.split_rhat_ess, a.runs)

    probs = (0.05, 0.5, 0.95)

    def host_route():
        x = ds.to_host()
        with ThreadPoolExecutor(a.threads) as ex:
            return list(ex.map(lambda p: ref.summary_param(x[:, :, p], probs), range(a.dim)))

    res["host_threads"] = a.threads
    res["host_runs"] = a.host_runs
    res["host_route_s"], res["host_route_all_s"] = timed(host_route, a.host_runs)
    m = 2 * a.chains * (a.draws // 2)
    res["sort_bytes"] = sort_bytes(m, a.dim, np.float32, gm.stats.sort_plan())
    res["device_faster_than_host"] = res["summary_s"] < res["host_route_s"]
    # the two routes on this sample, as a check that the timed work is the same work
    dev, host = ds.summary(), host_route()
    res["max_rhat_diff"] = float(np.nanmax(np.abs(dev.rhat - np.array([h["rhat"] for h in host]))))
    res["max_rel_ess_bulk_diff"] = float(np.nanmax(np.abs(dev.ess_bulk / np.array([h["ess_bulk"] for h in host]) - 1)))
    print(json.dumps(res))
    s.close()


if __name__ == "__main__":
    main()
