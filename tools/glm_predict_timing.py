"""Times GLM.predict on the samples of a run against the host route it replaces.

    python tools/glm_predict_timing.py                       # every shape, one JSON line each
    python tools/glm_predict_timing.py --dims 32 --dtypes f32 --rounds 3
    python tools/glm_predict_timing.py --only device ...     # warm-up + one call per shape (for a kernel trace)

Shape: --chains x --draws coefficient vectors from HMC.run_positions on a
Bernoulli-logit model of --rows rows, D in --dims, f32 and f64.
  arm A  target.predict(ds): the device route from the samples where they lie
         (validation, the model's upload and the result copy included)
  arm B  ds.to_host() and the numpy float64 transcription on --threads host
         threads, the copy included: blocks of draws, per block
         eta = theta X^T + offset, the link, ll, and streaming per-row sums
         (shifted sums for the moments, maximum-shifted sum for the lppd)
The arms alternate, --rounds rounds after one warm-up of arm A; medians and
ranges. The line also carries the largest difference of the two arms' outputs,
as a check that the timed work is the same work, and the product's 2 S M D
flops per second of arm A as a share of the vector peak (--peak-f32 / --peak-f64
TFLOP/s). The split of arm A into the main and the merge kernel comes from a
separate `rocprofv3 --kernel-trace --stats -- python tools/glm_predict_timing.py --only device`.
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


def host_route(ds, X, y, off, threads, block=2048):
    """The seven outputs from the host copy of the samples, numpy float64."""
    th = ds.to_host().reshape(-1, ds.dim)  # [chains * draws, D]; the reductions do not depend on the order
    S, M = th.shape[0], X.shape[0]
    Xt = np.ascontiguousarray(X.T)
    # pivots of the shifted sums: the first draw's values
    e0 = th[:1].astype(np.float64) @ Xt + off
    em0 = np.exp(-np.abs(e0))
    mu0 = np.where(e0 >= 0, 1.0, em0) / (1.0 + em0)
    l0 = y * e0 - (np.maximum(e0, 0.0) + np.log1p(em0))

    def part(lo):
        t = th[lo:lo + block].astype(np.float64)
        eta = t @ Xt + off
        em = np.exp(-np.abs(eta))
        A = np.maximum(eta, 0.0) + np.log1p(em)
        mu = np.where(eta >= 0, 1.0, em) / (1.0 + em)
        ll = y * eta - A
        r = []
        for v, p in ((eta, e0), (mu, mu0), (ll, l0)):
            d = v - p
            r += [d.sum(axis=0), np.einsum("ij,ij->j", d, d)]
        m = ll.max(axis=0)
        r += [m, np.exp(ll - m).sum(axis=0)]
        return r

    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(part, range(0, S, block)))
    out = {}
    for k, (name, p) in enumerate((("eta", e0), ("mu", mu0), ("ll", l0))):
        s1 = sum(q[2 * k] for q in parts)
        s2 = sum(q[2 * k + 1] for q in parts)
        out[name + "_mean"] = (p + s1 / S).reshape(M)
        var = ((s2 - s1 * s1 / S) / (S - 1)).reshape(M)
        out[name + ("_var" if name == "ll" else "_sd")] = var if name == "ll" else np.sqrt(var)
    m = np.max([q[6] for q in parts], axis=0)
    out["lppd"] = m + np.log(sum(q[7] * np.exp(q[6] - m) for q in parts)) - np.log(S)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--dims", default="32,128")
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threads", type=int, default=min(16, len(os.sched_getaffinity(0))))
    ap.add_argument("--peak-f32", type=float, default=157.3)
    ap.add_argument("--peak-f64", type=float, default=78.6)
    ap.add_argument("--only", choices=["device"], default=None)
    a = ap.parse_args()

    import general_mcmc_amd as gm
    from tests import _glm_ref

    for D in (int(v) for v in a.dims.split(",")):
        for name in a.dtypes.split(","):
            dtype = {"f32": np.float32, "f64": np.float64}[name]
            X, y, off = _glm_ref.synth(a.rows, D, "bernoulli_logit", 3)
            X, off = (v.astype(dtype).astype(np.float64) for v in (X, off))
            target = gm.GLM(X, y, family="bernoulli_logit", prior_sd=2.0, offset=off)
            x0 = (0.1 * gm.init_det(a.chains, D, np.float64)).astype(dtype)
            s = gm.HMC(target, x0, 0.02, 2, dtype=dtype).set_seed(42)
            ds = s.run_positions(a.draws, 10)
            s.synchronize()
            S = a.chains * a.draws
            dev = target.predict(ds)  # warm-up
            if a.only == "device":
                target.predict(ds)
                print(json.dumps({"only": "device", "dim": D, "dtype": name, "calls": 2}))
                s.close()
                continue
            ta, tb = [], []
            host = None
            for _ in range(a.rounds):
                t = time.perf_counter()
                dev = target.predict(ds)
                ta.append(time.perf_counter() - t)
                t = time.perf_counter()
                host = host_route(ds, X, y, off, a.threads)
                tb.append(time.perf_counter() - t)
            res = {"shape": [a.chains, a.draws, a.rows, D], "dtype": name, "rounds": a.rounds,
                   "host_threads": a.threads,
                   "device_s": statistics.median(ta), "device_range_s": [min(ta), max(ta)],
                   "host_s": statistics.median(tb), "host_range_s": [min(tb), max(tb)]}
            res["device_faster_than_host"] = max(ta) < min(tb)
            flops = 2.0 * S * a.rows * D
            peak = (a.peak_f32 if name == "f32" else a.peak_f64) * 1e12
            res["product_tflops_of_the_call"] = flops / res["device_s"] / 1e12
            res["share_of_vector_peak_of_the_call"] = flops / res["device_s"] / peak
            res["max_abs_diff"] = {k: float(np.max(np.abs(getattr(dev, k) - host[k]))) for k in host}
            print(json.dumps(res), flush=True)
            s.close()


if __name__ == "__main__":
    main()
