"""The identity-metric NUTS and the MH arithmetic tied to the reference's op
structure (CPU, oracle only).

The kernels sum every per-chain quantity in the engine's canonical order
(in-lane, then the lane butterfly) and evaluate exp / ln with their own
restatements of msun; the oracle's form 0 is that arithmetic, bit for bit
(the GPU parity tests). The oracle's form 1 is the reference as written:

* NUTS, identity metric (or_nuts_mass_run with mode 0, form 1): the kinetic
  energy `q = q + v * v` left to right (generic_nuts.rs:230-235), the U-turn
  dots `diff.dot(&vel)` left to right (:1369-1377; a burn tensor sum in the
  reference, euclidean.rs:400-403, whose order the backend picks), and the
  C library's exp / ln / pow where the reference calls f64::exp / ln / powf
  (the leaf's min(1, exp(joint - joint0)) :1197, the dual averaging
  :882-893, init_chain_state's mu :750, find_reasonable_epsilon's ln 0.5 and
  ln 2 :1072-1079).
* MH (or_mh_run form 1): MHMarkovChain::step (metropolis_hastings.rs:306-318)
  with IsotropicGaussian's logp (distributions.rs:378-390) and unnorm_logp
  (:398-406) as written: both sums left to right, log q forward and backward
  computed separately, the current state's log-density recomputed, and the
  accept's ln u and the proposal constant's ln from the C library.

Each form 1 is checked here against a pure-Python loop of the reference text
(bit for bit), and tied to form 0 by stated bounds:

  MH at cfg5's shape (IsotropicGaussian(1) 256-D f64, proposal sd 2.38/16),
  from identical states: |d log alpha| <= 1e-13 |lp'| (measured 3.2e-15) and
  <= 2e-12 absolute (measured 4.5e-13); accept decisions differing <= 0.1 %
  (measured 0 of 10,240).
  NUTS at cfg3's shape (the 32-D dense Gaussian, f64, identity metric): per
  chain final step size, tree length, accept count and per-coordinate mean and
  variance within 5 standard errors.

The GPU tests (tests/test_gpu_forms.py) tie the kernels to form 1 at the
configs' own sizes."""
import ctypes
import math

import numpy as np
import pytest

from tests import _nuts_ref
from tests._oracle import Target
from tests.test_oracle_nuts_forms import _mc_close, cfg3_target

_libm = ctypes.CDLL("libm.so.6")
for _f in ("exp", "log"):
    getattr(_libm, _f).restype = ctypes.c_double
    getattr(_libm, _f).argtypes = [ctypes.c_double]
_libm.pow.restype = ctypes.c_double
_libm.pow.argtypes = [ctypes.c_double, ctypes.c_double]

TAG_MH_PROP, TAG_MH_ACC = 4, 5


# --------------------------------------------------------------------- MH
def _ref_mh_run(oracle, std_t, x0, sd, seed, n_steps, collect_from):
    """metropolis_hastings.rs:306-318 with IsotropicGaussian as proposal and
    target, transcribed; the draws are the engine's RNG spec (the proposal
    normals of spec v5, the [0,1) accept uniform)."""
    lib = oracle.lib
    C_, D = x0.shape
    q = x0.copy()
    rows = []
    acc = np.zeros(C_, dtype=np.int64)

    def unnorm_logp(x):                      # distributions.rs:398-406
        s = 0.0
        for v in x:
            s = s + v * v
        return -0.5 * s / (std_t * std_t)

    def prop_logp(frm, to):                  # distributions.rs:378-390
        lp = 0.0
        d = float(len(frm))
        var = sd * sd
        for f, t in zip(frm, to):
            diff = t - f
            lp += -(diff * diff) / (2.0 * var)
        lp += -d * 0.5 * _libm.log(var * math.pi * sd * sd)
        return lp

    for s in range(n_steps):
        row = np.empty((C_, D))
        for c in range(C_):
            cur = [float(v) for v in q[c]]
            prop = [cur[i] + lib.or_tab_normal_d(seed, c, s, TAG_MH_PROP, i) * sd for i in range(D)]
            current_lp = unnorm_logp(cur)
            proposed_lp = unnorm_logp(prop)
            log_q_forward = prop_logp(cur, prop)
            log_q_backward = prop_logp(prop, cur)
            log_accept_ratio = (proposed_lp + log_q_backward) - (current_lp + log_q_forward)
            u = lib.or_uniform_co_d(seed, c, s, TAG_MH_ACC, 0)
            if log_accept_ratio > _libm.log(u):
                q[c] = prop
                acc[c] += 1
            row[c] = q[c]
        if s >= collect_from:
            rows.append(row)
    return q, np.array(rows), acc


def test_mh_reference_form_is_the_reference_text(oracle):
    rng = np.random.default_rng(5)
    C_, D, std_t, sd = 3, 7, 1.3, 0.45
    x0 = rng.standard_normal((C_, D)) * 1.3
    q, smp, acc = oracle.mh_run(Target(2, D, std=std_t), x0, sd, 11, 0, 40, 30, 8, 1, form=1)
    rq, rsmp, racc = _ref_mh_run(oracle, std_t, x0, sd, 11, 40, 30)
    np.testing.assert_array_equal(q, rq)
    np.testing.assert_array_equal(smp, rsmp)
    np.testing.assert_array_equal(acc, racc)
    assert 0 < acc.sum() < 40 * C_
    # and form 0 (the kernels' arithmetic) is a different computation
    la0, _, lnu0 = oracle.mh_terms(Target(2, D, std=std_t), x0, sd, 11, 0, 8, 1, 0)
    la1, _, lnu1 = oracle.mh_terms(Target(2, D, std=std_t), x0, sd, 11, 0, 8, 1, 1)
    assert np.all(np.abs(la0 - la1) <= 1e-13 * np.maximum(np.abs(la1), 1.0))


def test_mh_forms_tied_at_cfg5_shape(oracle):
    """cfg5's target and proposal, 512 chains (the GPU test runs 4096) after
    200 steps from N(0, 1): every 5th of 100 further steps, both forms from the
    same states."""
    C_, D, sd = 512, 256, 2.38 / 16
    t = Target(2, D, std=1.0)
    x0 = np.random.default_rng(0).standard_normal((C_, D))
    _, smp, _ = oracle.mh_run(t, x0, sd, 42, 0, 300, 200, 64, 4, threads=8)
    worst_rel = worst_abs = 0.0
    flips = n = 0
    for k in range(0, 100, 5):
        la0, lp0, lnu0 = oracle.mh_terms(t, smp[k], sd, 42, 300 + k, 64, 4, 0)
        la1, lp1, lnu1 = oracle.mh_terms(t, smp[k], sd, 42, 300 + k, 64, 4, 1)
        d = np.abs(la0 - la1)
        worst_abs = max(worst_abs, float(d.max()))
        worst_rel = max(worst_rel, float((d / np.abs(lp1)).max()))
        flips += int(np.sum((la0 > lnu0) != (la1 > lnu1)))
        n += C_
    assert worst_rel <= 1e-13 and worst_abs <= 2e-12, (worst_rel, worst_abs)
    assert flips <= 1e-3 * n, flips


def test_mh_run_forms_statistics(oracle):
    """run(100, 300) of both forms from the same start: per-coordinate means,
    variances and accept rates within 5 standard errors (64 chains, 32-D)."""
    C_, D, sd = 64, 32, 2.38 / math.sqrt(32)
    t = Target(2, D, std=1.0)
    x0 = np.random.default_rng(8).standard_normal((C_, D))
    res = []
    for form in (0, 1):
        _, smp, acc = oracle.mh_run(t, x0, sd, 3, 0, 400, 100, 32, 1, threads=8, form=form)
        res.append((smp.mean(axis=0), smp.var(axis=0), acc / 400.0))
    for a, b in zip(*res):
        assert _mc_close(a, b) < 5.0


# ------------------------------------------------------------------- NUTS
def _ref_nuts_run(oracle, t, lanes, elems, x0, eps0, n_collect, n_discard, seed, max_depth=10,
                  target_accept=0.8):
    """The transcription of identity-metric NUTS (tests/_nuts_ref.py) on a
    built-in target: the log-density is the oracle's."""
    return _nuts_ref.run(oracle, lambda q: oracle.logp_grad(t, q, lanes, elems, np.float64), x0, eps0, n_collect,
                         n_discard, seed, max_depth, target_accept)


@pytest.mark.parametrize("eps0", [-1.0, 0.3], ids=["find_eps", "given_eps"])
def test_nuts_identity_reference_form_is_the_reference_text(oracle, eps0):
    """6-D dense Gaussian, 3 chains, run(5, 4) (8 transitions: 4 of them
    adapting the step size), f64: the oracle's form 1 equals the transcription
    bit for bit -- samples, final positions, step-size state, accept and
    leapfrog counts."""
    rng = np.random.default_rng(21)
    d = 6
    a = rng.standard_normal((d, d))
    cov = a @ a.T / d + 0.3 * np.eye(d)
    t = Target(3, d, mean=rng.standard_normal(d) * 0.5, prec=np.linalg.inv(cov), norm_const=-2.0)
    C_ = 3
    x0 = rng.standard_normal((C_, d))
    st = oracle.nuts_state(C_, np.float64)
    st["eps"][:] = eps0
    q, smp, acc, nlf = oracle.nuts_run(t, x0, st, 0.8, 10, 17, 0, 5, 4, False, 8, 1, form=1)
    ref = _ref_nuts_run(oracle, t, 8, 1, x0, eps0, 5, 4, 17)
    for c in range(C_):
        np.testing.assert_array_equal(smp[:, c, :], ref[c]["samples"])
        np.testing.assert_array_equal(q[c], ref[c]["q"])
        assert st["eps"][c] == ref[c]["eps"] and st["eps_bar"][c] == ref[c]["eps_bar"]
        assert st["h_bar"][c] == ref[c]["h_bar"] and st["mu"][c] == ref[c]["mu"]
        assert acc[c] == ref[c]["acc"] and nlf[c] == ref[c]["nlf"]
    assert acc.sum() > 0 and nlf.min() >= 8
    # form 0 (the kernels' arithmetic) differs from it, slightly
    st0 = oracle.nuts_state(C_, np.float64)
    st0["eps"][:] = eps0
    q0, _, _, _ = oracle.nuts_run(t, x0, st0, 0.8, 10, 17, 0, 5, 4, False, 8, 1)
    assert not (np.array_equal(q0, q) and np.array_equal(st0["eps_bar"], st["eps_bar"]))


def test_nuts_identity_forms_statistics_cfg3_target(oracle):
    """cfg3's 32-D dense Gaussian under the identity metric, 64 chains,
    run(100, 300) of both forms from the same start (the GPU test runs the
    kernels against form 1 at 512 chains, run(500, 500)): per-chain final step
    size, tree length, accept count and per-coordinate mean and variance
    within 5 standard errors."""
    t = cfg3_target()
    C_, D = 64, 32
    x0 = np.random.default_rng(4).standard_normal((C_, D))
    res = []
    for form in (0, 1):
        st = oracle.nuts_state(C_, np.float64)
        _, smp, acc, nlf = oracle.nuts_run(t, x0, st, 0.8, 10, 9, 0, 100, 300, False, 16, 2, threads=8, form=form)
        res.append((st["eps_bar"].copy(), nlf / 399.0, acc, smp.mean(axis=0), smp.var(axis=0)))
    for x, y in zip(*res):
        assert _mc_close(x, y) < 5.0
    assert not np.array_equal(res[0][3], res[1][3])
