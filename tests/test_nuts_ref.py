"""The NUTS transcription (tests/_nuts_ref.py) as a reference for the GPU
(CPU, oracle only).

(a) The method on a target the oracle has: the oracle's form 0 is the
    kernels' arithmetic, which the GPU equals bit for bit (the parity tests),
    so put in the GPU's place it shows without a GPU that the kernels and the
    transcription differ by rounding only: the same trees, and a deviation
    within 16 times the transcription's own sensitivity to rounding.
(b) The GLM cases of tests/test_gpu_glm.py::test_nuts_follows_the_transcription
    through the transcription alone: the oracle's draws are the engine's, so
    every condition that test asserts about the transcription holds or fails
    here already.

The sensitivity (sens) is the deviation of the transcription from a second run
of itself whose log-density and gradient carry independent errors of the size
of the evaluation's derived forward bound. For the GLM that is
8 (N + D) u x GlmRef.scales (tests/test_gpu_glm.py, test 1). For the dense
Gaussian of (a), logp = c - 0.5 d'Pd and g = -Pd with d = x - mean: each entry
of Pd is a sum of D products, the quadratic form a further sum of D, so to first
order in any summation order |d g_j| <= 2 D u (|P| |d|)_j and
|d logp| <= 2 D u (0.5 |d|'|P||d| + |c|) (the rounding of d itself included);
with the GLM bound's factor 8 for the neglected terms, 16 D u x those scales.
"""
import numpy as np
import pytest

from tests import _glm_ref as R
from tests import _nuts_ref
from tests._oracle import Target


def _gauss_case():
    rng = np.random.default_rng(21)
    d = 6
    a = rng.standard_normal((d, d))
    cov = a @ a.T / d + 0.3 * np.eye(d)
    mean, prec = rng.standard_normal(d) * 0.5, np.linalg.inv(cov)
    return Target(3, d, mean=mean, prec=prec, norm_const=-2.0), mean, prec, rng.standard_normal((3, d))


@pytest.mark.parametrize("eps0", [-1.0, 0.3], ids=["find_eps", "given_eps"])
def test_form0_follows_the_transcription(oracle, eps0):
    t, mean, prec, x0 = _gauss_case()
    C_, d = x0.shape
    n_collect, n_discard, seed, lanes, elems = 5, 4, 17, 8, 1
    total = n_collect + n_discard - 1

    def logp_grad(q):
        return oracle.logp_grad(t, q, lanes, elems, np.float64)

    tol = 16.0 * d * R.unit_roundoff(np.float64)
    prng = np.random.default_rng(1)

    def perturbed(q):
        lp, g = logp_grad(q)
        ad = np.abs(q - mean)
        S = 0.5 * np.einsum("ci,ij,cj->c", ad, np.abs(prec), ad) + abs(t.norm_const)
        G = ad @ np.abs(prec)
        return lp + tol * S * prng.uniform(-1, 1, lp.shape), g + tol * G * prng.uniform(-1, 1, g.shape)

    r = _nuts_ref.stack(_nuts_ref.run(oracle, logp_grad, x0, eps0, n_collect, n_discard, seed))
    r2 = _nuts_ref.stack(_nuts_ref.run(oracle, perturbed, x0, eps0, n_collect, n_discard, seed))
    sens = _nuts_ref.deviation(r, r2)

    # form 0, whole run
    st = oracle.nuts_state(C_, np.float64)
    st["eps"][:] = eps0
    q, smp, acc, nlf = oracle.nuts_run(t, x0, st, 0.8, 10, seed, 0, n_collect, n_discard, False, lanes, elems)
    form0 = dict(samples=smp.transpose(1, 0, 2), q=q, eps=st["eps"], eps_bar=st["eps_bar"])
    # form 0, transition by transition, for the depths and the leapfrog counts: the run's init
    # (a run of no transition), then NUTS::step with the run's adaptation counter
    s1 = oracle.nuts_state(C_, np.float64)
    s1["eps"][:] = eps0
    q1, _, _, _ = oracle.nuts_run(t, x0, s1, 0.8, 10, seed, 0, 1, 0, False, lanes, elems)
    depth, n_leapfrog, accs = (np.zeros((C_, total), dtype=np.int64) for _ in range(3))
    for s in range(total):
        q1, accs[:, s], n_leapfrog[:, s], depth[:, s] = oracle.nuts_step_depth(
            t, q1, s1, 0.8, 10, seed, s, 1, s, n_discard, lanes, elems)
    np.testing.assert_array_equal(q1, q)  # the steps are the run
    np.testing.assert_array_equal(s1["eps_bar"], st["eps_bar"])
    np.testing.assert_array_equal(n_leapfrog.sum(axis=1), nlf)

    dev = _nuts_ref.deviation(form0, r)
    print(f"eps0 {eps0}: margin {r['margin'].min():.3e}, leapfrogs {r['nlf']}, depths up to {r['depth'].max()}, "
          f"sensitivity {sens:.3e}, form 0 deviation {dev:.3e}, ratio {dev / sens:.3f}")
    np.testing.assert_array_equal(depth, r["depth"])
    np.testing.assert_array_equal(n_leapfrog, r["n_leapfrog"])
    np.testing.assert_array_equal(acc, r["acc"])
    np.testing.assert_array_equal(accs.sum(axis=1), r["acc"])
    assert r["margin"].min() >= 1e-9, r["margin"]
    assert _nuts_ref.same_decisions(r, r2)
    assert sens > 0
    assert dev <= 16 * sens, (dev, sens)


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("shape", R.NUTS_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_glm_cases_meet_the_conditions_of_the_gpu_tie(oracle, shape, family):
    N, D, _ = shape
    r, r2, sens = R.nuts_reference(oracle, N, D, family)
    deep = r["depth"] >= 3
    print(f"{family} {N}x{D}: margin {r['margin'].min():.3e}, leapfrogs per chain {r['nlf']}, "
          f"depths up to {r['depth'].max()}, sensitivity {sens:.3e}")
    assert r["margin"].min() >= 1e-9, r["margin"]
    assert _nuts_ref.same_decisions(r, r2)          # stable under an evaluation error of the bound's size
    assert 0 < sens <= 1e-4                          # (posterior sds here are >= 0.05)
    # trees of depth >= 3 that doubled in both directions
    assert np.any(deep & (r["fwd"] > 0) & (r["fwd"] < r["depth"]))
    assert r["acc"].min() > 0


@pytest.mark.parametrize("family", R.FAMILIES)
def test_the_tolerance_sees_one_lost_partial(oracle, family):
    """What 16 sens can tell apart: a gradient whose column 32 (the second
    column chunk's only column at D = 33) loses the two rows of one lane's
    first float64 row vector, one of 150 such partials of one of 33 columns,
    moves the 300 x 33 run by more than the tolerance or changes its trees."""
    N, D = 300, 33
    ref, _, x0 = R.nuts_case(N, D, family)
    r, _, sens = R.nuts_reference(oracle, N, D, family)
    rows, col = [2, 3], 32  # lane 1's first rows at 64 lanes

    def lossy(q):
        lp, g = ref.logp_grad(q)
        _, mu = ref.link(ref.eta(q))
        g = g.copy()
        g[:, col] -= (ref.y[rows] - mu[:, rows]) @ ref.X[rows, col]
        return lp, g

    c = R.NUTS_RUN
    bad = _nuts_ref.stack(_nuts_ref.run(oracle, lossy, x0, -1.0, c["n_collect"], c["n_discard"], c["seed"],
                                        c["max_depth"], c["target_accept"]))
    dev = _nuts_ref.deviation(bad, r)
    print(f"{family}: one lost partial moves the run by {dev:.3e} = {dev / sens:.1e} sens")
    assert not _nuts_ref.same_decisions(bad, r) or dev > 16 * sens
