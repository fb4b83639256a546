"""Cost of the MH warm-up kernel (mh_adapt_kernel) next to the plain one at
bench.py's cfg5 shape: 16384 chains x 256-D IsotropicGaussian f64, proposal
std 2.38/16, 100 transitions per launch (CHAINS, DIM, ROUNDS override). Three
cases, device time from the run's HIP events, interleaved rounds, median and
range, in chain-steps per second:

  plain    mh_kernel
  frozen   mh_adapt_kernel MODE 0: per-chain scales all equal, all-ones shape
  warmup   mh_adapt_kernel MODE 2: a 100-transition mode-2 warm-up (start 5,
           end 10, first window 10: windows end at 15, 25, 45, 85 and 89, so
           the case includes the window updates and its launch cuts)

    python tools/probe_mh_adapt.py            # CASES=plain for a library without the new entry points
    python tools/probe_mh_adapt.py --ess      # efficiency on the badly scaled 8-D Gaussian instead

--ess: 4096 chains, run(1000, 1000) on N(0, diag(sigma^2)), sigma from 0.5 to
8: minimum bulk-ESS (Summary.ess_bulk) per second of device time of the
collection run, for the mode-2 and mode-1 warm-ups (from proposal std 1) and
for the fixed isotropic proposal stds 0.25, 0.5, 1, 2.
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import general_mcmc_amd as gm  # noqa: E402
from general_mcmc_amd import _lib  # noqa: E402

lib = _lib.load()
_lib.check(lib.gm_set_device(0))
_lib.require_gpu()


def cost():
    C_ = int(os.environ.get("CHAINS", "16384"))
    D_ = int(os.environ.get("DIM", "256"))
    N_, STD = 100, 2.38 / 16
    cases = tuple(os.environ.get("CASES", "plain,frozen,warmup").split(","))
    x0 = gm.init_with_seed(C_, D_, 42, np.float64)
    cfg = gm.MHAdaptConfig("diagonal", 0.234, 5, 10, 10, 0.05, 1e-6)

    def make(case):
        s = gm.MetropolisHastings(gm.IsotropicGaussian(1.0), gm.IsotropicGaussian(STD), x0).seed(42)
        s.reserve(N_)
        if case != "plain":
            s.set_proposal_scales(np.full(C_, STD))
        return s

    def one(case, s):
        """Device milliseconds of N_ transitions of `case`."""
        if case == "warmup":
            # the same start every round: positions, scales, shape and an armed warm-up
            s.set_positions(x0)
            s.set_proposal_scales(np.full(C_, STD)).set_proposal_diag(np.ones(D_)).set_adaptation(cfg)
            s.run_positions(0, N_)
        else:
            s.run_positions(N_, 0)
        return s.last_run_stats()[0]

    samplers = {c: make(c) for c in cases}
    t_end = time.perf_counter() + 0.3
    while time.perf_counter() < t_end:
        for c, s in samplers.items():
            one(c, s)
    res = {c: [] for c in cases}
    for _ in range(int(os.environ.get("ROUNDS", "9"))):
        for c, s in samplers.items():
            res[c].append(one(c, s))
    out = {"chains": C_, "dim": D_, "transitions": N_, "library": _lib.LIB_PATH}
    for c, v in res.items():
        ms = float(np.median(v))
        out[c] = {"median_ms": ms, "min_ms": float(np.min(v)), "max_ms": float(np.max(v)),
                  "chain_steps_per_s": C_ * N_ / (ms * 1e-3),
                  "chain_steps_per_s_range": [C_ * N_ / (float(np.max(v)) * 1e-3), C_ * N_ / (float(np.min(v)) * 1e-3)]}
    for c in ("frozen", "warmup"):
        if c in out and "plain" in out:
            out[c + "_over_plain"] = out[c]["median_ms"] / out["plain"]["median_ms"]
    print(json.dumps(out))


def ess():
    C_, D_, N_ = int(os.environ.get("CHAINS", "4096")), 8, 1000
    sigma = np.geomspace(0.5, 8.0, D_)
    mean, prec = np.zeros(D_), np.ascontiguousarray(np.diag(1.0 / sigma ** 2))

    class Target(gm.distributions._TargetBase):
        dim = D_

        def _fill(self, t, dim):
            t.kind = _lib.GM_TARGET_GAUSS
            t.mean = mean.ctypes.data_as(C.POINTER(C.c_double))
            t.prec = prec.ctypes.data_as(C.POINTER(C.c_double))
            t.norm_const = 0.0
            return [mean, prec]

    x0 = gm.init_with_seed(C_, D_, 42, np.float64)
    out = {"chains": C_, "dim": D_, "n_collect": N_, "n_discard": N_}
    arms = [("diagonal", 1.0), ("scale", 1.0)] + [("none", s) for s in (0.25, 0.5, 1.0, 2.0)]
    # untimed runs of the shape first: the first arm would otherwise be timed on a clock that is still ramping
    w = gm.MetropolisHastings(Target(), gm.IsotropicGaussian(1.0), x0).seed(7)
    t_end = time.perf_counter() + 0.3
    while time.perf_counter() < t_end:
        w.run_positions(N_, 0)
    w.close()
    for name, std in arms:
        s = gm.MetropolisHastings(Target(), gm.IsotropicGaussian(std), x0).seed(42)
        if name != "none":
            s.set_adaptation(gm.MHAdaptConfig(name))
        s.run_positions(0, N_)     # the warm-up (plain burn-in for the fixed arms)
        ds = s.run_positions(N_, 0)
        ms = s.last_run_stats()[0]
        e = float(np.min(ds.summary().ess_bulk))
        key = name if name != "none" else f"fixed_{std}"
        out[key] = {"min_ess_bulk": e, "device_ms": ms, "min_ess_bulk_per_s": e / (ms * 1e-3),
                    "median_scale": float(np.median(s.proposal_scales()[0]))}
        s.close()
    best = max(v["min_ess_bulk_per_s"] for k, v in out.items() if k.startswith("fixed_"))
    out["diagonal_over_best_fixed"] = out["diagonal"]["min_ess_bulk_per_s"] / best
    out["scale_over_best_fixed"] = out["scale"]["min_ess_bulk_per_s"] / best
    print(json.dumps(out))


if __name__ == "__main__":
    ess() if "--ess" in sys.argv[1:] else cost()
