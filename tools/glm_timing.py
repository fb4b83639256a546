"""Times frozen HMC (L = 10) and NUTS on a synthetic logistic regression,
N = 1024 rows by D = 32 columns, on two arms in one process:

  glm     the GLM target (gm.GLM, glm_device.h)
  custom  a CustomTarget transcription of the same model with X, y, the offset
          and the prior in `params`: one chain per lane, every lane walks every
          row (the only route before the GLM target existed)

    python tools/glm_timing.py                       # all shapes, one JSON line each
    python tools/glm_timing.py --chains 4096 --dtypes float32 --samplers hmc

Per shape (C chains, dtype, sampler): both arms' logp / gradient are checked
against the numpy reference on the timed data within the bound of
tests/test_gpu_glm.py (8 (N + D) u scale); each arm is warmed up, then timed in
--rounds alternating rounds, a round repeating runs until their device time
(the samplers' own event pairs, Sampler.last_run_stats) reaches --min-time.
A NUTS run starts from its step-size search and adapts the step size over its
transitions, in both arms alike; its leapfrogs are the samplers' own counts.
Printed: chain-leapfrogs/s, achieved flop/s, the share of the vector peak
(157.3 TFLOP/s f32, half of it f64), and glm/custom with its range over rounds.
Flops per chain-leapfrog, from the shapes: 4 N D (two multiply-adds per matrix
entry) + 8 N for the link (exp counted as one) and the residual.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.custom_targets import GLM as CUSTOM_SOURCE  # noqa: E402

PEAK = {"float32": 157.3e12, "float64": 78.65e12}


def flops_per_leapfrog(N, D):
    return 4 * N * D + 8 * N


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--chains", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--dtypes", nargs="+", default=["float32", "float64"])
    ap.add_argument("--samplers", nargs="+", default=["hmc", "nuts"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-time", type=float, default=0.5)
    ap.add_argument("--layout", type=int, nargs=2, default=None, help="the GLM arm's layout (lanes elems)")
    a = ap.parse_args()

    import general_mcmc_amd as gm
    from tests import _glm_ref as R

    N, D = a.rows, a.dim
    X, y, off = R.synth(N, D, "bernoulli_logit", 1)
    sd = np.full(D, 2.0)
    ref = R.GlmRef(X, y, "bernoulli_logit", sd, off)
    glm = gm.GLM(X, y, prior_sd=sd, offset=off)
    custom = gm.CustomTarget(CUSTOM_SOURCE, D, np.concatenate([[N, 1.0], 1.0 / sd ** 2, off, y, X.ravel()]))
    arms = {"glm": glm, "custom": custom}
    fl = flops_per_leapfrog(N, D)

    for dtype_name in a.dtypes:
        dtype = np.dtype(dtype_name).type
        # both arms compute the model, within the tests' bound, on the timed data
        th = (0.3 * gm.init_with_seed(70, D, 5, np.float64)).astype(dtype)
        rr = ref.rounded(dtype)
        lp_ref, g_ref = rr.logp_grad(th.astype(np.float64))
        S, G = rr.scales(th.astype(np.float64))
        tol = 8.0 * (N + D) * R.unit_roundoff(dtype)
        agree = {}
        for name, t in arms.items():
            lp, g = t.unnorm_logp_and_grad_batch(th, dtype)
            agree[name] = [float(np.max(np.abs(lp - lp_ref) / (tol * S))), float(np.max(np.abs(g - g_ref) / (tol * G)))]
            if max(agree[name]) > 1.0:
                raise SystemExit(f"{name} arm misses the evaluation bound on the timed shape: {agree[name]}")
        for C_ in a.chains:
            x0 = (0.3 * gm.init_with_seed(C_, D, 7, np.float64)).astype(dtype)
            for sampler in a.samplers:
                def make(t):
                    if sampler == "hmc":
                        s = gm.HMC(t, x0, 0.02, 10, dtype=dtype)
                    else:
                        s = gm.NUTS(t, x0, 0.8, dtype=dtype)
                    s.set_seed(3)
                    if a.layout and t is glm:
                        s.set_layout(*a.layout)
                    return s

                ss = {n: make(t) for n, t in arms.items()}
                steps = 20 if sampler == "hmc" else 10

                def one(s):
                    """(device seconds, chain-leapfrogs) of one run of `steps` transitions."""
                    before = s.leapfrog_counts().sum() if sampler == "nuts" else 0
                    s.run_positions(1 if sampler == "nuts" else 0, steps)  # (a NUTS run collects at least a row)
                    ms, _ = s.last_run_stats()
                    lf = (s.leapfrog_counts().sum() - before) if sampler == "nuts" else C_ * steps * 10
                    return ms * 1e-3, float(lf)

                for s in ss.values():  # warm-up: compiles the custom kernels, NUTS finds its step size
                    one(s)
                rates = {n: [] for n in ss}
                for _ in range(a.rounds):
                    for n, s in ss.items():
                        t = lf = 0.0
                        while t < a.min_time:
                            dt_, l_ = one(s)
                            t += dt_
                            lf += l_
                        rates[n].append(lf / t)
                ratio = [g_ / c_ for g_, c_ in zip(rates["glm"], rates["custom"])]
                res = {"rows": N, "dim": D, "chains": C_, "dtype": dtype_name, "sampler": sampler,
                       "glm_layout": list(ss["glm"].layout()), "flops_per_leapfrog": fl, "eval_vs_bound": agree}
                for n in ss:
                    med = statistics.median(rates[n])
                    res[n] = {"chain_leapfrogs_per_s": med, "range": [min(rates[n]), max(rates[n])],
                              "flops_per_s": med * fl, "share_of_vector_peak": med * fl / PEAK[dtype_name]}
                res["glm_over_custom"] = {"median": statistics.median(ratio), "range": [min(ratio), max(ratio)]}
                print(json.dumps(res), flush=True)
                for s in ss.values():
                    s.close()


if __name__ == "__main__":
    main()
