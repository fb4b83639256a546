"""What the NUTS metric conventions buy on cfg3's target (32-D Gaussian,
eigenvalues 0.1 ... 10, random rotation), 8192 chains, f64.

Arms: identity (NUTS::new), reference dense (M = Sigma_hat per chain, the
reference's convention), whitening per-chain dense (M^-1 = Sigma_hat per
chain), whitening pooled dense (one Sigma_hat from all chains). Each arm runs
400 warm-up transitions (run_positions(1, 400), default windows) and then
collects 400 (run_positions(400, 0)); reported per arm: median eps_bar after
the warm-up, leapfrogs per collected transition, device time of the warm-up
and of the collection (the runs' HIP events), summary().ess_bulk.min() of the
collection and that per second of its device time. The arms alternate within
this process, ROUNDS (5) times, a fresh sampler with the same seed each time,
so the samples repeat and the spread is the timing's: median with min - max.

Read the device's clocks beside a run (rocm-smi --showclocks, before and
after) and quote them with the figures.

    python tools/probe_nuts_metric.py
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
ROUNDS = int(os.environ.get("ROUNDS", "5"))
CHAINS = int(os.environ.get("CHAINS", "8192"))
N_WARM = N_COLLECT = 400
MEAN, COV = bench.dense_gauss_32()
ARMS = {
    "identity": None,
    "reference_dense": gm.NUTSMassMatrixConfig("dense"),
    "whitening_per_chain": gm.NUTSMassMatrixConfig("dense", convention="whitening"),
    "whitening_pooled": gm.NUTSMassMatrixConfig("dense", convention="whitening", pooled=True),
}


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def one(cfg):
    target = gm.DenseGaussian(MEAN, COV)
    x0 = gm.init_with_seed(CHAINS, 32, 23, np.float64)
    s = gm.NUTS(target, x0, 0.8, dtype=np.float64) if cfg is None else gm.NUTS.new_with_mass_matrix(
        target, x0, 0.8, cfg, dtype=np.float64)
    s.set_seed(31)
    s.run_positions(1, N_WARM)
    warm_ms = s.last_run_stats()[0]
    eps_bar = float(np.median(s.step_sizes()[1]))
    lf0 = s.leapfrog_counts().sum()
    dev = s.run_positions(N_COLLECT, 0)
    ms = s.last_run_stats()[0]
    lf = float(s.leapfrog_counts().sum() - lf0) / (CHAINS * (N_COLLECT - 1))
    ess = float(np.min(dev.summary().ess_bulk))
    row = {"median_eps_bar": eps_bar, "leapfrogs_per_transition": lf, "warmup_ms": warm_ms, "collect_ms": ms,
           "min_ess_bulk": ess, "min_ess_bulk_per_s": ess / (ms * 1e-3)}
    if cfg is not None and cfg.pooled:
        row["updates"], row["failed"] = s.metric_updates()
    del dev
    s.close()
    return row


if __name__ == "__main__":
    rows = {k: [] for k in ARMS}
    for _ in range(ROUNDS):
        for k, cfg in ARMS.items():
            rows[k].append(one(cfg))
    for k, v in rows.items():
        print(json.dumps(dict(arm=k, chains=CHAINS, n_warmup=N_WARM, n_collect=N_COLLECT, rounds=ROUNDS,
                              **{name: spread([r[name] for r in v]) for name in v[0]})), flush=True)
    for k in ("whitening_per_chain", "whitening_pooled"):
        for base in ("identity", "reference_dense"):
            ratio = [a["min_ess_bulk_per_s"] / b["min_ess_bulk_per_s"] for a, b in zip(rows[k], rows[base])]
            print(json.dumps({f"{k}_over_{base}_min_ess_bulk_per_s": spread(ratio)}), flush=True)
