"""Cost of the dense-metric HMC kernel (hmc_dense_kernel) next to the plain and
the diagonal-metric ones, and what the dense warm-up buys on cfg3's target.

Cost: device time from the run's HIP events, interleaved rounds (ROUNDS, 9),
median with min and max, in chain-leapfrogs per second, at two shapes. A timed
run is one launch of n transitions that stores the last one only; n is sized
per case from a calibration run so that the run takes about WINDOW_MS (250)
milliseconds of device time:
  cfg2    4096 chains x 64-D Rosenbrock f32, L = 50
  gauss   8192 chains x 32-D DenseGaussian f64 (cfg3's target), L = 10
Cases: plain (hmc_kernel), diag (hmc_adapt_kernel MODE 0, identity metric),
dense (hmc_dense_kernel MODE 0, identity metric).

Benefit (BUYS=1): cfg3's target, 8192 chains f64. Each warm-up ("diagonal",
"dense"; L = 3, eps0 = 0.5, run(0, 400)) gives eps_bar and a metric; L is then
chosen so that median(eps_bar) * L * omega is nearest pi / 2, omega the
frequency of the slowest direction under that metric; a sampler with that L
and the frozen step sizes and metric collects 400 transitions:
summary().ess_bulk.min() per second of device time. The two arms collect in
alternation, BUYS_ROUNDS (5) times each, every collection continuing its chain;
median, min and max over the rounds are reported, and the ratio of the medians.

Read the device's clocks beside a run (rocm-smi --showclocks, before and
after) and quote them with the figures.

    python tools/probe_hmc_dense.py
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import general_mcmc_amd as gm  # noqa: E402
from general_mcmc_amd import _lib  # noqa: E402

lib = _lib.load()
_lib.check(lib.gm_set_device(0))
_lib.require_gpu()
N_CAL = 100
ROUNDS = int(os.environ.get("ROUNDS", "9"))
WINDOW_MS = float(os.environ.get("WINDOW_MS", "250"))
BUYS_ROUNDS = int(os.environ.get("BUYS_ROUNDS", "5"))
MEAN, COV = bench.dense_gauss_32()


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def cost(name, target, chains, dim, dtype, eps, n_leapfrog):
    x0 = (gm.init_with_seed(chains, dim, 42, np.float64) * 0.5).astype(dtype)

    def make(case):
        s = gm.HMC(target, x0, eps, n_leapfrog, dtype=dtype).set_seed(42)
        s.reserve(1)
        if case == "diag":
            s.set_step_sizes(np.full(chains, eps))
        if case == "dense":
            s.set_dense_metric(np.eye(dim))
        return s

    def one(s, n):
        s.run_positions(1, n - 1)
        return s.last_run_stats()[0]

    cases = ("plain", "diag", "dense")
    samplers = {c: make(c) for c in cases}
    # warm-up and calibration: transitions per timed run for about WINDOW_MS of device time
    n_of = {}
    for c, s in samplers.items():
        one(s, N_CAL)
        n_of[c] = max(N_CAL, int(WINDOW_MS / (one(s, N_CAL) / N_CAL)))
        one(s, n_of[c])
    res = {c: [] for c in cases}
    for _ in range(ROUNDS):
        for c, s in samplers.items():
            res[c].append(one(s, n_of[c]) / n_of[c])  # ms per transition
    out = {"shape": name, "chains": chains, "dim": dim, "dtype": np.dtype(dtype).name, "n_leapfrog": n_leapfrog,
           "rounds": ROUNDS}
    for c, v in res.items():
        ms = float(np.median(v))
        out[c] = {"transitions_per_run": n_of[c], "run_ms": ms * n_of[c], "median_ms": ms,
                  "min_ms": float(np.min(v)), "max_ms": float(np.max(v)),
                  "chain_leapfrogs_per_s": chains * n_leapfrog / (ms * 1e-3)}
    out["dense_over_plain"] = out["dense"]["median_ms"] / out["plain"]["median_ms"]
    out["dense_over_diag"] = out["dense"]["median_ms"] / out["diag"]["median_ms"]
    for s in samplers.values():
        s.close()
    print(json.dumps(out), flush=True)


def buys_arm(kind, chains, target):
    """The warm-up of `kind` and a sampler frozen at what it found."""
    x0 = gm.init_with_seed(chains, 32, 23, np.float64)
    w = gm.HMC.with_adaptation(target, x0, 0.5, 3, gm.HMCAdaptConfig(kind), dtype=np.float64).set_seed(31)
    w.run(0, 400)
    eps_bar = w.step_sizes()[1]
    if kind == "dense":
        minv = w.dense_metric()[0]
        lt = np.linalg.cholesky(minv)
        white = np.linalg.solve(lt, np.linalg.solve(lt, COV).T)  # L^-1 Sigma L^-T
    else:
        dinv = np.median(w.metric()[0], axis=0)
        white = COV / np.sqrt(np.outer(dinv, dinv))
    omega = 1.0 / np.sqrt(np.linalg.eigvalsh(0.5 * (white + white.T)).max())  # the slowest direction
    med = float(np.median(eps_bar))
    n_leapfrog = max(1, int(round(np.pi / 2 / (med * omega))))
    s = gm.HMC(target, w.positions(), 0.5, n_leapfrog, dtype=np.float64).set_seed(32)
    s.set_step_sizes(eps_bar)
    if kind == "dense":
        s.set_dense_metric(minv)
    else:
        s.set_metric(w.metric()[0])
    w.close()
    return s, {"warmup": kind, "n_leapfrog": n_leapfrog, "median_eps_bar": med, "omega_slowest": float(omega)}


def buys(chains=8192, n_collect=400):
    target = gm.DenseGaussian(MEAN, COV)
    arms = {k: buys_arm(k, chains, target) for k in ("diagonal", "dense")}
    rows = {k: {"acceptance": [], "device_ms": [], "min_ess_bulk": [], "min_ess_bulk_per_s": []} for k in arms}
    for _ in range(BUYS_ROUNDS):
        for k, (s, _) in arms.items():
            dev = s.run_positions(n_collect, 0)
            ms = s.last_run_stats()[0]
            out = dev.to_host()
            ess = float(np.min(dev.summary().ess_bulk))
            r = rows[k]
            r["acceptance"].append(float(np.mean(np.any(out[:, 1:] != out[:, :-1], axis=2))))
            r["device_ms"].append(ms)
            r["min_ess_bulk"].append(ess)
            r["min_ess_bulk_per_s"].append(ess / (ms * 1e-3))
            del dev, out
    for k, (s, info) in arms.items():
        print(json.dumps(dict(info, chains=chains, n_collect=n_collect, rounds=BUYS_ROUNDS,
                              **{name: spread(v) for name, v in rows[k].items()})), flush=True)
        s.close()
    ratio = [d / g for d, g in zip(rows["dense"]["min_ess_bulk_per_s"], rows["diagonal"]["min_ess_bulk_per_s"])]
    print(json.dumps({"dense_over_diagonal_min_ess_bulk_per_s": spread(ratio)}), flush=True)


if __name__ == "__main__":
    cost("cfg2", gm.RosenbrockND(), 4096, 64, np.float32, 0.01, 50)
    cost("gauss", gm.DenseGaussian(MEAN, COV), 8192, 32, np.float64, 0.1, 10)
    if os.environ.get("BUYS", "0") == "1":
        buys()
