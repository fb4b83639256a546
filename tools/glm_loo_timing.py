"""Times GLM.loo on the samples of a run against the host route it replaces.

    python tools/glm_loo_timing.py                          # every shape, one JSON line each
    python tools/glm_loo_timing.py --dims 32 --dtypes f32 --rows 64 --rounds 3
    python tools/glm_loo_timing.py --only device ...        # warm-up + one call per shape (for a kernel trace)

Shape: --chains x --draws coefficient vectors from HMC.run_positions on a
Bernoulli-logit model, D in --dims, f32 and f64, data rows in --rows.
  arm A  target.loo(ds): the device route from the samples where they lie (the
         predict call for the lppd, validation, the model's upload and the
         result copies included); the time of target.predict(ds) alone beside it
  arm B  ds.to_host() and the numpy float64 transcription (tests/_glm_loo_ref.py)
         on --threads host threads, the copy included: ll = y eta - A in blocks
         of draws, then one row per task (a sort of all S values each).
         Only for row counts up to --host-rows (64): 1024 rows would take
         sixteen times as long, many minutes, and are not run; nothing is
         extrapolated.
The arms alternate, --rounds rounds after one warm-up of arm A; medians and
ranges. The line also carries the largest difference of the two arms' outputs,
as a check that the timed work is the same work. The split of arm A into its
kernels comes from a separate
`rocprofv3 --kernel-trace --stats -- python tools/glm_loo_timing.py --only device`.
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


def host_route(ds, X, y, off, threads, block=65536):
    """elpd_loo and pareto_k from the host copy of the samples, numpy float64."""
    from tests import _glm_loo_ref as L
    th = ds.to_host().reshape(-1, ds.dim)  # [chains * draws, D]; the result does not depend on the order
    S, N = th.shape[0], X.shape[0]
    Xt = np.ascontiguousarray(X.T)
    ll = np.empty((N, S))

    def part(lo):
        eta = th[lo:lo + block].astype(np.float64) @ Xt + off
        ll[:, lo:lo + block] = (y * eta - (np.maximum(eta, 0.0) + np.log1p(np.exp(-np.abs(eta))))).T

    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(part, range(0, S, block)))
        rows = list(ex.map(lambda i: L.psis_row(ll[i])[:2], range(N)))
    return {"elpd_loo": np.array([r[0] for r in rows]), "pareto_k": np.array([r[1] for r in rows])}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--rows", default="64,1024")
    ap.add_argument("--host-rows", type=int, default=64)
    ap.add_argument("--dims", default="32,128")
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threads", type=int, default=min(16, len(os.sched_getaffinity(0))))
    ap.add_argument("--only", choices=["device"], default=None)
    a = ap.parse_args()

    import general_mcmc_amd as gm
    from tests import _glm_ref

    for D in (int(v) for v in a.dims.split(",")):
        for name in a.dtypes.split(","):
            dtype = {"f32": np.float32, "f64": np.float64}[name]
            for N in (int(v) for v in a.rows.split(",")):
                X, y, off = _glm_ref.synth(N, D, "bernoulli_logit", 3)
                X, off = (v.astype(dtype).astype(np.float64) for v in (X, off))
                target = gm.GLM(X, y, family="bernoulli_logit", prior_sd=2.0, offset=off)
                x0 = (0.1 * gm.init_det(a.chains, D, np.float64)).astype(dtype)
                s = gm.HMC(target, x0, 0.02, 2, dtype=dtype).set_seed(42)
                ds = s.run_positions(a.draws, 10)
                s.synchronize()
                dev = target.loo(ds)  # warm-up
                if a.only == "device":
                    target.loo(ds)
                    print(json.dumps({"only": "device", "dim": D, "dtype": name, "rows": N, "calls": 2}), flush=True)
                    s.close()
                    continue
                with_host = N <= a.host_rows
                ta, tp, tb = [], [], []
                host = None
                for _ in range(a.rounds):
                    t = time.perf_counter()
                    dev = target.loo(ds)
                    ta.append(time.perf_counter() - t)
                    t = time.perf_counter()
                    target.predict(ds)
                    tp.append(time.perf_counter() - t)
                    if with_host:
                        t = time.perf_counter()
                        host = host_route(ds, X, y, off, a.threads)
                        tb.append(time.perf_counter() - t)
                res = {"shape": [a.chains, a.draws, N, D], "dtype": name, "rounds": a.rounds,
                       "tail_len": dev.tail_len, "group_rows": gm.stats.loo_plan(dtype, a.chains * a.draws, N)["group_rows"],
                       "device_s": statistics.median(ta), "device_range_s": [min(ta), max(ta)],
                       "predict_alone_s": statistics.median(tp), "predict_alone_range_s": [min(tp), max(tp)],
                       "k_range": [float(np.min(dev.pareto_k)), float(np.max(dev.pareto_k))], "p_loo": dev.p_loo}
                if with_host:
                    res.update({"host_threads": a.threads, "host_s": statistics.median(tb),
                                "host_range_s": [min(tb), max(tb)], "device_faster_than_host": max(ta) < min(tb),
                                "host_over_device": statistics.median(tb) / statistics.median(ta),
                                "max_abs_diff": {k: float(np.max(np.abs(getattr(dev, k) - host[k]))) for k in host}})
                print(json.dumps(res), flush=True)
                s.close()


if __name__ == "__main__":
    main()
