"""Cost of the HMC warm-up kernel (hmc_adapt_kernel) next to the plain one at
the cfg2 shape: 4096 chains x 64-D Rosenbrock f32, L = 50, 100 transitions
per launch (CHAINS, DIM, ROUNDS override). Three cases, device time from the
run's HIP events, interleaved rounds, median, in chain-leapfrogs per second:

  plain    hmc_kernel
  frozen   hmc_adapt_kernel MODE 0: per-chain step sizes all equal, identity metric
  warmup   hmc_adapt_kernel MODE 2: a 100-transition mode-2 warm-up (start 5,
           end 10, first window 10: windows end at 15, 25, 45, 85 and 89, so
           the case includes the window updates and its launch cuts)

    python tools/probe_hmc_adapt.py
"""
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
C_ = int(os.environ.get("CHAINS", "4096"))
D_ = int(os.environ.get("DIM", "64"))
L_, N_, EPS = 50, 100, 0.01
x0 = gm.init_with_seed(C_, D_, 42, np.float64).astype(np.float32)
CFG = gm.HMCAdaptConfig("diagonal", 0.8, 5, 10, 10, 0.05, 1e-6)


def make(case):
    s = gm.HMC(gm.RosenbrockND(), x0, EPS, L_).set_seed(42)
    s.reserve(N_)
    if case != "plain":
        s.set_step_sizes(np.full(C_, EPS))
    return s


def one(case, s):
    """Device milliseconds of N_ transitions of `case`."""
    if case == "warmup":
        # the same start every round: positions, step sizes and an armed warm-up
        s.set_positions(x0)
        s.set_step_sizes(np.full(C_, EPS)).set_metric(np.ones(D_, dtype=np.float32)).set_adaptation(CFG)
        s.run_positions(0, N_)
    else:
        s.run_positions(N_, 0)
    return s.last_run_stats()[0]


cases = ("plain", "frozen", "warmup")
samplers = {c: make(c) for c in cases}
t_end = time.perf_counter() + 0.3
while time.perf_counter() < t_end:
    for c, s in samplers.items():
        one(c, s)
res = {c: [] for c in cases}
for _ in range(int(os.environ.get("ROUNDS", "15"))):
    for c, s in samplers.items():
        res[c].append(one(c, s))
out = {"chains": C_, "dim": D_, "n_leapfrog": L_, "transitions": N_}
for c, v in res.items():
    ms = float(np.median(v))
    out[c] = {"median_ms": ms, "min_ms": float(np.min(v)), "max_ms": float(np.max(v)),
              "chain_leapfrogs_per_s": C_ * L_ * N_ / (ms * 1e-3)}
out["frozen_over_plain"] = out["frozen"]["median_ms"] / out["plain"]["median_ms"]
out["warmup_over_plain"] = out["warmup"]["median_ms"] / out["plain"]["median_ms"]
print(json.dumps(out))
