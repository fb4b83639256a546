"""The GLM target (gm.GLM; glm_device.h) on the GPU.

1. evaluation parity with the numpy float64 reference (tests/_glm_ref.py);
2. every compiled layout: the same bound, and results that do not depend on
   where a chain sits in the grid;
3. HMC follows the float64 transcription (tests/_hmc_adapt_ref.py, mode 0)
   driven by the engine's own draws;
4. the HMC warm-up and NUTS do what they are for;
5. engine properties: reproducible, checkpoint/resume, sharding, statistics;
6. the refusals.

The bound of 1 and 2, with u the dtype's unit roundoff,
    |d logp| <= 8 (N + D) u S,   |d g_j| <= 8 (N + D) u G_j
(S, G: _glm_ref.GlmRef.scales) is the first-order forward error of the sums in
any summation order with a factor 8 for the link function and the neglected
terms: derived, not measured.
"""
import ctypes as C

import numpy as np
import pytest

from tests import _glm_ref as R
from tests import _hmc_adapt_ref as href

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
SHAPES = [(1, 1), (7, 3), (64, 16), (65, 17), (257, 33), (100, 128), (1000, 5)]
LAYOUTS = [(16, 2), (64, 1), (64, 2)]  # GM_GLM_LAYOUT_LIST (glm_layouts.h)
N_CHAINS = 70


def _case(N, D, family, seed):
    """(reference, gm.GLM arguments, theta [70, D]): X ~ N(0, 1/D), offset ~ 0.3 N(0, 1), |theta_j| ~ 2."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D)) / np.sqrt(D)
    off = 0.3 * rng.standard_normal(N)
    sd = rng.uniform(0.5, 3.0, D)
    y = (rng.random(N) < 0.4).astype(np.float64) if family == "bernoulli_logit" else rng.poisson(2.0, N).astype(
        np.float64)
    theta = 2.0 * rng.standard_normal((N_CHAINS, D))
    return R.GlmRef(X, y, family, sd, off), dict(X=X, y=y, family=family, prior_sd=sd, offset=off), theta


def _check_bound(ref, dtype, theta_t, lp, g, what):
    """theta_t: the positions as the device holds them (dtype)."""
    rr = ref.rounded(dtype)
    th = theta_t.astype(np.float64)
    lp_ref, g_ref = rr.logp_grad(th)
    S, G = rr.scales(th)
    tol = 8.0 * (ref.N + ref.D) * R.unit_roundoff(dtype)
    r_lp = float(np.max(np.abs(lp.astype(np.float64) - lp_ref) / (tol * S)))
    print(f"{what}: |d logp| / bound = {r_lp:.3e}", end="")
    if g is not None:
        r_g = float(np.max(np.abs(g.astype(np.float64) - g_ref) / (tol * G)))
        print(f", |d g| / bound = {r_g:.3e}", end="")
    print()
    assert np.all(np.isfinite(lp))
    assert r_lp <= 1.0
    if g is not None:
        assert np.all(np.isfinite(g))
        assert r_g <= 1.0


# ---- 1. evaluation parity ------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("shape", SHAPES)
def test_evaluation_parity(gm, shape, family, dtype):
    N, D = shape
    ref, kw, theta = _case(N, D, family, 100 + N + D)
    x = theta.astype(dtype)
    lp, g = gm.GLM(**kw).unnorm_logp_and_grad_batch(x, dtype)
    assert lp.dtype == dtype and g.shape == (N_CHAINS, D)
    _check_bound(ref, dtype, x, lp, g, f"{family} {N}x{D} {np.dtype(dtype).name}")


def test_bernoulli_rows_at_eta_800_stay_finite(gm):
    rng = np.random.default_rng(5)
    X = rng.standard_normal((9, 2))
    X[3] = [800.0, 0.0]
    X[6] = [-800.0, 0.0]
    y = (rng.random(9) < 0.5).astype(np.float64)
    y[3], y[6] = 0.0, 1.0  # the rows where the asymptote is the whole term
    ref = R.GlmRef(X, y, "bernoulli_logit", 2.0)
    theta = np.array([[1.0, 0.3], [-1.0, 0.2]])
    lp, g = gm.GLM(X, y, prior_sd=2.0).unnorm_logp_and_grad_batch(theta, np.float64)
    _check_bound(ref, np.float64, theta, lp, g, "eta = +-800")
    assert lp[0] < -1500  # chain 0 pays both rows' 800


# ---- 2. every compiled layout ----------------------------------------------------
def _engine_draws(gm, n_chains, dim, seed, n):
    """The momentum normals and accept uniforms of transitions 0..n-1 of a
    float64 sampler with this seed (chain ids 0..n_chains-1)."""
    from general_mcmc_amd import batch_vector as bv
    z = bv.DeviceMatrix((n_chains, dim), np.float64)
    zs, us = [], []
    for t in range(n):
        bv.fill_random_normal(z, seed, t)
        zs.append(z.to_host())
        us.append(bv.sample_uniform(n_chains, np.float64, seed, t).to_host())
    return lambda t: (zs[t], us[t])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_layout_logp(gm, layout, family, dtype):
    """A sampler's log-density of its start positions (no leapfrog: the
    transition evaluates them and proposes them again) at each layout."""
    ref, kw, theta = _case(65, 17, family, 7)
    x = theta.astype(dtype)
    s = gm.HMC(gm.GLM(**kw), x, 0.1, 0, dtype=dtype).set_seed(1).set_layout(*layout)
    assert s.layout() == layout
    s.run(0, 1)
    np.testing.assert_array_equal(s.positions(), x)
    _check_bound(ref, dtype, x, s.logp(), None, f"layout {layout} {family} {np.dtype(dtype).name}")
    s.close()


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_layout_gradient(gm, layout, family):
    """The gradient at each layout, read back from one leapfrog of an accepted
    float64 transition with the engine's own momentum z:
    q1 = q + eps (z + (eps/2) g(q)), so g = ((q1 - q)/eps - z) 2/eps. Its
    rounding, a few u |q| / eps^2 = 64 u |q|, is far inside the bound
    (8 * 82 u G_j with G_j of the order of the column's absolute sum)."""
    seed, eps = 3, 0.25
    ref, kw, theta = _case(65, 17, family, 7)
    x = 0.25 * theta  # near the mode: most proposals are accepted
    s = gm.HMC(gm.GLM(**kw), x, eps, 1, dtype=np.float64).set_seed(seed).set_layout(*layout)
    out = s.run(1, 0)[:, 0]
    acc = s.accept_counts() == 1
    assert acc.sum() >= N_CHAINS // 2, acc.sum()
    z, _ = _engine_draws(gm, N_CHAINS, 17, seed, 1)(0)
    g = ((out - x) / eps - z) * (2.0 / eps)
    rr = ref.rounded(np.float64)
    _, g_ref = rr.logp_grad(x)
    _, G = rr.scales(x)
    tol = 8.0 * (65 + 17) * R.unit_roundoff(np.float64)
    ratio = float(np.max((np.abs(g - g_ref) / (tol * G))[acc]))
    print(f"layout {layout} {family}: |d g| / bound = {ratio:.3e} over {acc.sum()} accepted chains")
    assert ratio <= 1.0
    _check_bound(ref, np.float64, out, s.logp(), None, f"layout {layout} {family} logp after the step")
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sampler", ["hmc", "nuts"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_results_do_not_depend_on_the_place_in_the_grid(gm, layout, sampler, dtype):
    """Global chain 69 as the only chain, as the last of 63, and as the first of 70."""
    _, kw, _ = _case(65, 17, "bernoulli_logit", 7)
    target = gm.GLM(**kw)
    k = 69
    x_all = (0.3 * gm.init_with_seed(k + 70, 17, 21, np.float64)).astype(dtype)
    rows = []
    for first, n in ((k, 1), (k - 62, 63), (k, 70)):
        x0 = x_all[first:first + n]
        if sampler == "hmc":
            s = gm.HMC(target, x0, 0.1, 3, dtype=dtype, chain_offset=first)
        else:
            s = gm.NUTS(target, x0, 0.8, dtype=dtype, chain_offset=first)
        s.set_seed(9).set_layout(*layout)
        rows.append(s.run(3, 2)[k - first])
        s.close()
    assert np.all(np.isfinite(rows[0])) and np.any(rows[0][0] != rows[0][-1])
    np.testing.assert_array_equal(rows[0], rows[1])
    np.testing.assert_array_equal(rows[0], rows[2])


# ---- 3. HMC follows the transcription ----------------------------------------------
# Column scale of X per family, chosen on the CPU with the transcription under
# numpy's draws (seeds 0..4) so that at eps = 0.05, L = 4 it accepts 60-85 % of
# its proposals with every decision at least 5e-6 from its threshold; the test
# asserts the conditions themselves for the engine's draws.
_HMC_XSCALE = {"bernoulli_logit": 8.0, "poisson_log": 0.7}


def _hmc_case(family, xs=1.0):
    N, D = 40, 5
    rng = np.random.default_rng(17)
    X = rng.standard_normal((N, D)) * xs
    off = 0.3 * rng.standard_normal(N)
    th = 0.5 * rng.standard_normal(D) / xs
    eta = X @ th + off
    if family == "bernoulli_logit":
        y = (rng.random(N) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    else:
        y = rng.poisson(np.exp(eta)).astype(np.float64)
    return R.GlmRef(X, y, family, 2.0, off), dict(X=X, y=y, family=family, prior_sd=2.0, offset=off)


@pytest.mark.parametrize("family", R.FAMILIES)
def test_hmc_follows_the_transcription(gm, family):
    n_chains, dim, n_leapfrog, eps, n_collect, n_discard = 6, 5, 4, 0.05, 20, 10
    seed = 29
    xs = _HMC_XSCALE[family]
    ref, kw = _hmc_case(family, xs)
    x0 = 1.5 * gm.init_with_seed(n_chains, dim, 14, np.float64) / (xs if family == "bernoulli_logit" else 1.0)
    draws = _engine_draws(gm, n_chains, dim, seed, n_collect + n_discard)
    s = gm.HMC(gm.GLM(**kw), x0, eps, n_leapfrog, dtype=np.float64).set_seed(seed)
    out = s.run(n_collect, n_discard)
    r = href.run(ref.logp_grad, x0, eps, n_leapfrog, n_collect, n_discard, 0, draws)

    # the transcription's own sensitivity: a second run whose logp and gradient carry independent
    # errors of the size of test 1's bound
    prng = np.random.default_rng(1)
    tol = 8.0 * (ref.N + ref.D) * R.unit_roundoff(np.float64)

    def perturbed(q):
        lp, g = ref.logp_grad(q)
        S, G = ref.scales(q)
        with np.errstate(invalid="ignore"):  # (a rejected overflow: infinite scales)
            return (lp + tol * S * prng.uniform(-1, 1, lp.shape), g + tol * G * prng.uniform(-1, 1, g.shape))

    r2 = href.run(perturbed, x0, eps, n_leapfrog, n_collect, n_discard, 0, draws)
    sens = max(float(np.max(np.abs(r["q"] - r2["q"]))), float(np.max(np.abs(r["samples"] - r2["samples"]))))
    dev = max(float(np.max(np.abs(s.positions() - r["q"]))), float(np.max(np.abs(out - r["samples"]))))
    n_acc = int(r["accepted"].sum())
    print(f"{family}: margin {r['margin']:.3e}, accepted {n_acc} of {r['accepted'].size}, "
          f"sensitivity {sens:.3e}, GPU deviation {dev:.3e}")
    assert r["margin"] >= 1e-9, r["margin"]
    assert 0 < n_acc < r["accepted"].size  # both accept and reject occur
    np.testing.assert_array_equal(r["accepted"], r2["accepted"])
    np.testing.assert_array_equal(s.accept_counts(), r["accepted"].sum(axis=0))
    moved = np.any(out[:, 1:] != out[:, :-1], axis=2)
    np.testing.assert_array_equal(moved, r["accepted"][n_discard + 1:].T)
    assert sens > 0
    assert dev <= 16 * sens, (dev, sens)
    s.close()


# ---- 4. warm-up and NUTS do what they are for ---------------------------------------
def _moves(samples):
    return float(np.mean(np.any(samples[:, 1:] != samples[:, :-1], axis=2)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_hmc_warmup_on_badly_scaled_columns(gm, dtype):
    """Poisson regression whose columns' scales spread 0.1 .. 10: after the
    diagonal warm-up the sampling-phase acceptance sits in the band of
    test_gpu_hmc_adapt.py's badly scaled Gaussian (mode 2: 0.78 .. 0.98), and
    the chains agree (rank-normalised R-hat below 1.01, the threshold of
    Vehtari et al. 2021 for the 256 x 200 draws).

    L = 3: with the adapted metric every coordinate of the near-Gaussian
    posterior oscillates at frequency 1, and that test's band for the adapted
    step size at this dim is 0.45 .. 0.8, so eps * L is 1.35 .. 2.4: from about
    a quarter period (the best decorrelation) to well short of the half period
    pi, where a fixed-L trajectory maps q to -q, and of 2 pi, where it returns
    to its start (L = 10 puts eps * L at 4.5 .. 8 around 2 pi: the float64
    transcription, tests/_hmc_adapt_ref.py under numpy's draws, ends at
    eps = 0.635 and R-hat 1.08 - 1.13 there, and at R-hat 0.999 with L = 3).
    regularize = 0: the default adds 0.05 to every variance, 300 times the
    narrowest posterior variance here (1.6e-4), which would put back the bad
    scaling the warm-up is to remove; the transcription with it off finds the
    variances 0.53 .. 1.4e-4 and accepts 0.90 of its sampling proposals."""
    n_chains, D, N = 256, 8, 200
    rng = np.random.default_rng(23)
    scales = np.geomspace(0.1, 10.0, D)
    X = rng.standard_normal((N, D)) * scales / np.sqrt(D)
    th = 0.5 * rng.standard_normal(D) / scales
    off = np.full(N, 1.0)
    y = rng.poisson(np.exp(X @ th + off)).astype(np.float64)
    target = gm.GLM(X, y, family="poisson_log", prior_sd=1.0, offset=off)
    x0 = (0.01 * gm.init_with_seed(n_chains, D, 20, np.float64)).astype(dtype)
    cfg = gm.HMCAdaptConfig("diagonal", 0.8, 75, 50, 25, 0.0, 1e-6)
    s = gm.HMC.with_adaptation(target, x0, 0.01, 3, cfg, dtype=dtype).set_seed(31)
    dev = s.run_positions(200, 400)
    out = dev.to_host().astype(np.float64)
    summ = dev.summary()
    acc = _moves(out)
    dinv = np.median(s.metric()[0].astype(np.float64), axis=0)
    print(f"acceptance {acc:.3f}, max R-hat {float(np.max(summ.rhat)):.4f}, median dinv {dinv}, "
          f"posterior sd {summ.sd}")
    assert np.all(np.isfinite(out))
    assert 0.78 <= acc <= 0.98
    assert float(np.max(summ.rhat)) < 1.01
    # the metric found the columns' scales: the variances span at least (10 / 0.1)^2 / 100
    assert dinv[0] / dinv[-1] > 100.0
    s.close()


def _quadrature_mean(ref, n, lim=8.0):
    t = np.linspace(-lim, lim, n)
    a, b = np.meshgrid(t, t, indexing="ij")
    lp, _ = ref.logp_grad(np.stack([a.ravel(), b.ravel()], axis=1))
    w = np.exp(lp - lp.max())
    w /= w.sum()
    return np.array([np.sum(w * a.ravel()), np.sum(w * b.ravel())])


@pytest.mark.parametrize("dtype", DTYPES)
def test_nuts_posterior_mean_against_quadrature(gm, dtype):
    N, D, n_chains = 30, 2, 256
    rng = np.random.default_rng(41)
    X = np.stack([np.ones(N), rng.standard_normal(N)], axis=1)
    y = (rng.random(N) < 1.0 / (1.0 + np.exp(-(0.5 + X[:, 1])))).astype(np.float64)
    ref = R.GlmRef(X, y, "bernoulli_logit", 2.0)
    mean = _quadrature_mean(ref, 400)
    assert np.max(np.abs(mean - _quadrature_mean(ref, 799))) < 1e-6  # the grid is converged
    x0 = (0.5 * gm.init_with_seed(n_chains, D, 22, np.float64)).astype(dtype)
    s = gm.NUTS.new_with_mass_matrix(gm.GLM(X, y, prior_sd=2.0), x0, 0.8, gm.NUTSMassMatrixConfig(),
                                     dtype=dtype).set_seed(5)
    summ = s.run_positions(150, 150).summary()
    err = np.abs(summ.mean - mean)
    bound = 5.0 * summ.sd / np.sqrt(summ.ess_bulk)
    print(f"NUTS mean {summ.mean}, quadrature {mean}, |diff| {err}, bound {bound}, ess_bulk {summ.ess_bulk}")
    assert np.all(err <= bound)
    s.close()


# ---- 5. engine properties -----------------------------------------------------------
def _make(gm, sampler, target, x0, dtype, chain_offset=0):
    if sampler == "hmc":
        s = gm.HMC(target, x0, 0.1, 4, dtype=dtype, chain_offset=chain_offset)
    elif sampler == "hmc_adapt":
        s = gm.HMC.with_adaptation(target, x0, 0.1, 4, gm.HMCAdaptConfig("diagonal", 0.8, 5, 10, 10, 0.05, 1e-6),
                                   dtype=dtype, chain_offset=chain_offset)
    elif sampler == "nuts":
        s = gm.NUTS(target, x0, 0.8, dtype=dtype, chain_offset=chain_offset)
    else:
        s = gm.NUTS.new_with_mass_matrix(target, x0, 0.8, gm.NUTSMassMatrixConfig("diagonal", 5, 10, 10), dtype=dtype,
                                         chain_offset=chain_offset)
    return s.set_seed(12)


def _prop_target(gm, family="bernoulli_logit"):
    _, kw = _hmc_case(family)
    return gm.GLM(**kw)


SAMPLERS = ["hmc", "hmc_adapt", "nuts", "nuts_diag"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_same_seed_same_bits_and_sharding(gm, sampler, dtype):
    target = _prop_target(gm)
    x0 = (0.3 * gm.init_with_seed(16, 5, 3, np.float64)).astype(dtype)
    a, b = _make(gm, sampler, target, x0, dtype), _make(gm, sampler, target, x0, dtype)
    half = _make(gm, sampler, target, x0[:8], dtype)
    out = a.run(6, 40)
    assert np.all(np.isfinite(out)) and np.any(out[:, 0] != out[:, -1])
    np.testing.assert_array_equal(out, b.run(6, 40))
    np.testing.assert_array_equal(out[:8], half.run(6, 40))
    for s in (a, b, half):
        s.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_checkpoint_resumes_bit_for_bit(gm, sampler, dtype):
    target = _prop_target(gm, "poisson_log")
    x0 = (0.3 * gm.init_with_seed(12, 5, 4, np.float64)).astype(dtype)
    a = _make(gm, sampler, target, x0, dtype)
    a.run(3, 40)
    blob = a.save_state()
    b = _make(gm, sampler, target, x0, dtype).load_state(blob)
    np.testing.assert_array_equal(a.run(5, 0), b.run(5, 0))
    np.testing.assert_array_equal(a.positions(), b.positions())
    assert a.save_state() == b.save_state()
    a.close()
    b.close()


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_collect_stats_leaves_the_samples_unchanged(gm, sampler):
    target = _prop_target(gm)
    x0 = 0.3 * gm.init_with_seed(10, 5, 6, np.float64)
    a, b = _make(gm, sampler, target, x0, np.float64), _make(gm, sampler, target, x0, np.float64)
    b.collect_stats(True)
    out = a.run(6, 40)
    np.testing.assert_array_equal(out, b.run(6, 40))
    st = b.last_stats().summary()
    assert st.n_transitions >= 5 and np.all(st.mean_accept_stat > 0)
    a.close()
    b.close()


@pytest.mark.parametrize("sampler", ["hmc_adapt", "nuts_diag"])
def test_progress_and_device_resident_runs_are_the_plain_run(gm, sampler):
    target = _prop_target(gm)
    x0 = 0.3 * gm.init_with_seed(10, 5, 9, np.float64)
    a, b, c = (_make(gm, sampler, target, x0, np.float64) for _ in range(3))
    out = a.run(6, 40)
    seen = []
    out_b, stats = b.run_progress(6, 40, progress=seen.append, interval=0.0)
    if sampler.startswith("nuts"):
        # NUTS.run's row 0 is the state after n_discard - 1 transitions (the reference's count),
        # run_progress's the state after n_discard + 1: the same chain one row apart
        np.testing.assert_array_equal(out[:, 1:], out_b[:, :-1])
    else:
        np.testing.assert_array_equal(out, out_b)
    assert stats is not None and seen and seen[-1].done == seen[-1].total
    np.testing.assert_array_equal(out, c.set_steps_per_launch(7).run_positions(6, 40).to_host())
    for s in (a, b, c):
        s.close()


def test_hmc_step_sizes_and_metric_are_taken(gm):
    """A chain with its own step size and metric is the one-chain sampler with them."""
    target = _prop_target(gm)
    n = 9
    x0 = 0.3 * gm.init_with_seed(n, 5, 10, np.float64)
    eps = 0.05 * (1.0 + np.arange(n) / 8.0)
    minv = np.tile(np.array([1.0, 0.25, 4.0, 0.5, 2.0]), (n, 1)) * (1.0 + np.arange(n)[:, None])
    s = gm.HMC(target, x0, 0.05, 4, dtype=np.float64).set_seed(8).set_step_sizes(eps).set_metric(minv)
    out = s.run(5, 3)
    np.testing.assert_array_equal(s.step_sizes()[0], eps)
    np.testing.assert_array_equal(s.metric()[0], minv)
    for c in (0, 4, 8):
        one = gm.HMC(target, x0[c:c + 1], 0.05, 4, dtype=np.float64, chain_offset=c).set_seed(8)
        one.set_step_sizes(eps[c:c + 1]).set_metric(minv[c:c + 1])
        np.testing.assert_array_equal(one.run(5, 3)[0], out[c])
        one.close()
    assert np.any(out[:, 0] != out[:, -1])
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_poisson_overflow_is_not_clamped(gm, dtype):
    """eta past the exp range: the log-density is not finite, and a chain that
    proposes such a point stays where it is."""
    X = np.array([[1.0], [2.0], [0.5]])
    y = np.array([1.0, 0.0, 3.0])
    target = gm.GLM(X, y, family="poisson_log", prior_sd=1e3)
    lp, g = target.unnorm_logp_and_grad_batch(np.array([[800.0], [0.1]]), dtype)
    assert not np.isfinite(lp[0]) and np.isfinite(lp[1])
    assert lp[0] == -np.inf or np.isnan(lp[0])
    x0 = np.full((4, 1), 0.1, dtype=dtype)
    s = gm.HMC(target, x0, 300.0, 1, dtype=dtype).set_seed(2)  # one step of 300 overshoots into the overflow
    out = s.run(3, 0)
    np.testing.assert_array_equal(out, np.broadcast_to(x0[:, None, :], out.shape))
    assert s.accept_counts().sum() == 0
    s.close()


# ---- 6. refusals --------------------------------------------------------------------
def test_refusals(gm):
    L = gm._lib
    lib = L.load()
    _, kw = _hmc_case("bernoulli_logit")
    target = gm.GLM(**kw)
    x0 = 0.3 * gm.init_with_seed(4, 5, 8, np.float64)

    def refused(fn):
        with pytest.raises(gm.GMError) as e:
            fn()
        assert e.value.code == L.GM_EINVAL and "GLM target" in str(e.value), str(e.value)

    # MH, a hundred times over: a refused sampler leaves nothing behind
    for _ in range(100):
        refused(lambda: gm.MetropolisHastings(target, gm.IsotropicGaussian(0.5), x0))
    refused(lambda: gm.batch_vector.BatchTarget(target, 5, np.float64))
    h = gm.HMC(target, x0, 0.1, 3)
    refused(lambda: h.set_adaptation(gm.HMCAdaptConfig("dense")))
    refused(lambda: h.set_dense_metric(np.eye(5)))
    refused(lambda: h.set_layout(128, 4))   # wide
    refused(lambda: h.set_layout(32, 1))    # not one of the target's layouts
    n = gm.NUTS(target, x0, 0.8)
    refused(lambda: n.set_mass_adaptation(gm.NUTSMassMatrixConfig("dense")))
    refused(lambda: n.set_mass_adaptation(gm.NUTSMassMatrixConfig("diagonal", convention="whitening", pooled=True)))
    refused(lambda: n.set_layout(128, 4))
    # the C side's validation, with the facade's wording
    t, keep = target.to_struct(5)
    t.dim = 200
    out = C.c_void_p()
    big = np.zeros((4, 200))
    assert lib.gm_hmc_create(C.byref(t), 1, 4, 200, L.ptr(big), 0.1, 3, 0, C.byref(out)) == L.GM_EINVAL
    assert b"GLM target: dim must be in [1, 128]" in lib.gm_last_error()
    bad = kw["y"].copy()
    bad[7] = 2.0
    t2, keep2 = target.to_struct(5)
    t2.glm.contents.y = bad.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.gm_hmc_create(C.byref(t2), 1, 4, 5, L.ptr(x0), 0.1, 3, 0, C.byref(out)) == L.GM_EINVAL
    assert b"bernoulli_logit needs 0 <= y <= 1 at row 7" in lib.gm_last_error()
    # and both samplers still run
    assert np.all(np.isfinite(h.run(2, 1))) and np.all(np.isfinite(n.run(2, 1)))
    # the whitening convention per chain is supported
    n.set_mass_adaptation(gm.NUTSMassMatrixConfig("diagonal", 5, 10, 10, convention="whitening"))
    assert np.all(np.isfinite(n.run(2, 40)))
    h.close()
    n.close()
