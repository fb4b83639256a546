"""The GLM target (gm.GLM; glm_device.h) on the GPU.

1. evaluation parity with the numpy float64 reference (tests/_glm_ref.py);
2. every compiled layout: the same bound, and results that do not depend on
   where a chain sits in the grid;
3. HMC and its warm-up follow the float64 transcription
   (tests/_hmc_adapt_ref.py, modes 0, 1, 2) driven by the engine's own draws,
   and NUTS follows its own (tests/_nuts_ref.py), at up to four column chunks;
4. the HMC warm-up and NUTS do what they are for;
5. engine properties: reproducible, checkpoint/resume, sharding, statistics;
6. the refusals.

The bound of 1 and 2, with u the dtype's unit roundoff,
    |d logp| <= 8 (N + D) u S,   |d g_j| <= 8 (N + D) u G_j
(S, G: _glm_ref.GlmRef.scales) is the first-order forward error of the sums in
any summation order with a factor 8 for the link function and the neglected
terms: derived, not measured.

The ties of 3 share one tolerance. dev is the largest deviation of the GPU from
the float64 transcription; sens is the deviation of the transcription from a
second run of itself whose log-density and gradient carry independent errors
of the size of that bound (_glm_ref.perturbed); dev <= 16 sens is asserted,
after three conditions on the inputs, for the engine's draws: every decision
of the transcription at least 1e-9 from its threshold, the perturbed run
making the same decisions, and sens <= 1e-4 (the posterior sds are >= 0.05),
so that the tolerance can never grow to the size of a real error. Positions
are compared absolutely (they are of order 1: prior sd 2, starts 0.3 N(0, 1)),
step sizes and metrics relative to their values.

The evaluation takes GLM_CH = 32 gradient columns per pass over the rows and
one LDS exchange per glm_xc<T>() columns; a lane's second coordinate slot holds
a coordinate once D > 64; the f32 64-lane layouts walk 256 rows per pass. The
shapes past one chunk (WIDE), each the smallest that reaches its path, at
6 chains (four chains per block at 64 lanes: the second block is partly empty):
    300 x 33   a second chunk; two row passes in f32
    70 x 64    a full 64 x 1 layout
    70 x 65    the default layout becomes 64 x 2, lane 0's second slot is real,
               a third chunk
    300 x 128  four chunks, every slot real
"""
import ctypes as C
import time

import numpy as np
import pytest

from tests import _glm_ref as R
from tests import _hmc_adapt_ref as href
from tests import _nuts_ref
from tests import custom_targets as ct

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
SHAPES = [(1, 1), (7, 3), (64, 16), (65, 17), (257, 33), (100, 128), (1000, 5)]
LAYOUTS = [(16, 2), (64, 1), (64, 2)]  # GM_GLM_LAYOUT_LIST (glm_layouts.h)
N_CHAINS = 70
WIDE = [(300, 33), (70, 64), (70, 65), (300, 128)]  # (N, D)
N_WIDE_CHAINS = 6
# (N, D, layout): the default layout and every other one that admits the shape
WIDE_LAYOUTS = [(N, D, lay) for N, D in WIDE for lay in ((64, 1), (64, 2)) if lay[0] * lay[1] >= D]


def _default_layout(D):
    return (64, 1) if D <= 64 else (64, 2)


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
def _engine_draws(gm, n_chains, dim, seed, n, dtype=np.float64):
    """The momentum normals and accept uniforms of transitions 0..n-1 of a
    sampler of this dtype with this seed (chain ids 0..n_chains-1)."""
    from general_mcmc_amd import batch_vector as bv
    z = bv.DeviceMatrix((n_chains, dim), dtype)
    zs, us = [], []
    for t in range(n):
        bv.fill_random_normal(z, seed, t)
        zs.append(z.to_host())
        us.append(bv.sample_uniform(n_chains, dtype, seed, t).to_host())
    return lambda t: (zs[t], us[t])


def _layout_case(N, D, family):
    """65 x 17 with its 70 chains, the WIDE shapes with 6."""
    ref, kw, theta = _case(N, D, family, 7)
    return ref, kw, theta if (N, D) == (65, 17) else theta[:N_WIDE_CHAINS]


def _layout_logp(gm, N, D, layout, family, dtype):
    ref, kw, theta = _layout_case(N, D, family)
    x = theta.astype(dtype)
    s = gm.HMC(gm.GLM(**kw), x, 0.1, 0, dtype=dtype).set_seed(1)
    if D > 32:
        assert s.layout() == _default_layout(D)
    s.set_layout(*layout)
    assert s.layout() == layout
    s.run(0, 1)
    np.testing.assert_array_equal(s.positions(), x)
    _check_bound(ref, dtype, x, s.logp(), None, f"{N}x{D} layout {layout} {family} {np.dtype(dtype).name}")
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_layout_logp(gm, layout, family, dtype):
    """A sampler's log-density of its start positions (no leapfrog: the
    transition evaluates them and proposes them again) at each layout."""
    _layout_logp(gm, 65, 17, layout, family, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("case", WIDE_LAYOUTS, ids=lambda c: f"{c[0]}x{c[1]}-{c[2][0]}x{c[2][1]}")
def test_every_layout_logp_past_one_chunk(gm, case, family, dtype):
    N, D, layout = case
    _layout_logp(gm, N, D, layout, family, dtype)


def _layout_gradient(gm, N, D, layout, family, dtype):
    seed, eps = 3, 0.25
    ref, kw, theta = _layout_case(N, D, family)
    n_chains = theta.shape[0]
    x = (0.25 * theta).astype(dtype)  # near the mode: most proposals are accepted
    s = gm.HMC(gm.GLM(**kw), x, eps, 1, dtype=dtype).set_seed(seed).set_layout(*layout)
    out = s.run(1, 0)[:, 0]
    acc = s.accept_counts() == 1
    assert acc.sum() >= n_chains // 2, acc.sum()
    z, _ = _engine_draws(gm, n_chains, D, seed, 1, dtype)(0)
    assert z.dtype == dtype
    x64, out64 = x.astype(np.float64), out.astype(np.float64)
    g = ((out64 - x64) / eps - z.astype(np.float64)) * (2.0 / eps)
    rr = ref.rounded(dtype)
    _, g_ref = rr.logp_grad(x64)
    _, G = rr.scales(x64)
    tol = R.bound(ref, dtype)
    u = R.unit_roundoff(dtype)
    # the read-back's own rounding is inside the bound, coordinate by coordinate
    readback = 2.0 * u * np.abs(x64) / eps ** 2 + 2.0 * u * np.abs(z) / eps
    print(f"{N}x{D} layout {layout} {family} {np.dtype(dtype).name}: read-back rounding / bound = "
          f"{float(np.max(readback / (tol * G))):.3e}", end=", ")
    assert np.all(readback <= 0.1 * tol * G)
    ratio = float(np.max((np.abs(g - g_ref) / (tol * G))[acc]))
    print(f"|d g| / bound = {ratio:.3e} over {acc.sum()} accepted chains")
    assert ratio <= 1.0
    _check_bound(ref, dtype, out, s.logp(), None, f"layout {layout} {family} logp after the step")
    s.close()


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_layout_gradient(gm, layout, family):
    """The gradient at each layout, read back from one leapfrog of an accepted
    transition with the engine's own momentum z (drawn in the sampler's dtype):
    q1 = q + eps (z + (eps/2) g(q)), so g = ((q1 - q)/eps - z) 2/eps, computed in
    float64 from the device's values. Its own rounding: q1 is rounded once,
    u |q|, which the read-back multiplies by 2/eps^2, and so is the half-kicked
    momentum, u |z|, multiplied by 2/eps: 2 u |q| / eps^2 + 2 u |z| / eps, in
    either dtype a multiple of the same u as the bound. At eps = 0.25 that is
    32 u |q| + 8 u |z|, about 50 u for |q| ~ 0.5 and |z| <= 4, against the bound
    8 (N + D) u G_j with G_j of the order of the column's absolute sum:
    656 u G_j at 65 x 17, 1072 u G_j .. 3424 u G_j at the shapes past one chunk,
    and G_j >= 10 at all of them: under half a percent of the bound. The test
    asserts that it stays below a tenth of the bound at every coordinate."""
    _layout_gradient(gm, 65, 17, layout, family, np.float64)


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_layout_gradient_f32(gm, layout, family):
    """test_every_layout_gradient in float32: the momenta from a float32 DeviceMatrix."""
    _layout_gradient(gm, 65, 17, layout, family, np.float32)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("case", WIDE_LAYOUTS, ids=lambda c: f"{c[0]}x{c[1]}-{c[2][0]}x{c[2][1]}")
def test_every_layout_gradient_past_one_chunk(gm, case, family, dtype):
    """test_every_layout_gradient at 2 - 4 column chunks, LOGP = false inside the leapfrog."""
    N, D, layout = case
    _layout_gradient(gm, N, D, layout, family, dtype)


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


# Past one column chunk: tests/_glm_ref.synth's data (seed 3, prior sd 2), 6 chains from
# 0.3 N(0, 1), L = 4. The step sizes were chosen on the CPU with the transcription under the
# engine's draws (the oracle library restates them) so that both accept and reject occur and
# the three conditions on the inputs hold; the tests assert all of that for the draws they get.
_WIDE_HMC_EPS = {"bernoulli_logit": 0.25, "poisson_log": 0.08}
_WIDE_HMC_SEED = 29


def _wide_hmc_case(gm, N, D, family):
    X, y, off = R.synth(N, D, family, 3)
    x0 = 0.3 * gm.init_with_seed(N_WIDE_CHAINS, D, 14, np.float64)
    return R.GlmRef(X, y, family, 2.0, off), dict(X=X, y=y, family=family, prior_sd=2.0, offset=off), x0


_HMC_DEV_KEYS = {0: (), 1: ("eps", "eps_bar"), 2: ("eps", "eps_bar", "dinv")}


def _hmc_dev(a, b, mode):
    """Positions absolute, step sizes and metric relative to b's."""
    d = [np.max(np.abs(a["q"] - b["q"])), np.max(np.abs(a["samples"] - b["samples"]))]
    d += [np.max(np.abs(a[k] - b[k]) / np.abs(b[k])) for k in _HMC_DEV_KEYS[mode]]
    return float(max(d))


def _hmc_reference(ref, x0, eps, L, n_collect, n_discard, mode, draws, adapt=()):
    """(transcription, its perturbed second run, sens) -- no GPU work."""
    args = (x0, eps, L, n_collect, n_discard, mode, draws) + tuple(adapt)
    r = href.run(ref.logp_grad, *args)
    r2 = href.run(R.perturbed(ref, R.bound(ref, np.float64)), *args)
    return r, r2, _hmc_dev(r2, r, mode)


def _assert_hmc_tie(what, gpu, r, r2, sens, mode, n_discard):
    dev = _hmc_dev(gpu, r, mode)
    n_acc = int(r["accepted"].sum())
    print(f"{what}: margin {r['margin']:.3e}, accepted {n_acc} of {r['accepted'].size}, sensitivity {sens:.3e}, "
          f"GPU deviation {dev:.3e}, dev / sens {dev / sens:.1e}")
    assert r["margin"] >= 1e-9, r["margin"]
    assert 0 < n_acc < r["accepted"].size  # both accept and reject occur
    np.testing.assert_array_equal(r["accepted"], r2["accepted"])
    assert 0 < sens <= 1e-4, sens
    np.testing.assert_array_equal(gpu["acc"], r["accepted"].sum(axis=0))
    moved = np.any(gpu["samples"][:, 1:] != gpu["samples"][:, :-1], axis=2)
    np.testing.assert_array_equal(moved, r["accepted"][n_discard + 1:].T)
    assert dev <= 16 * sens, (dev, sens)


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("shape", [(300, 33), (300, 128)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_hmc_follows_the_transcription_past_one_chunk(gm, shape, family):
    """hmc_adapt_kernel<f64, 64, E, GlmT, 0> at two and at four column chunks."""
    N, D = shape
    L, eps, n_collect, n_discard = 4, _WIDE_HMC_EPS[family], 12, 6
    ref, kw, x0 = _wide_hmc_case(gm, N, D, family)
    draws = _engine_draws(gm, N_WIDE_CHAINS, D, _WIDE_HMC_SEED, n_collect + n_discard)
    s = gm.HMC(gm.GLM(**kw), x0, eps, L, dtype=np.float64).set_seed(_WIDE_HMC_SEED)
    assert s.layout() == _default_layout(D)
    out = s.run(n_collect, n_discard)
    gpu = dict(q=s.positions(), samples=out, acc=s.accept_counts())
    s.close()
    r, r2, sens = _hmc_reference(ref, x0, eps, L, n_collect, n_discard, 0, draws)
    _assert_hmc_tie(f"{family} {N}x{D}", gpu, r, r2, sens, 0, n_discard)


# The warm-up kept short, because the recurrence amplifies differences (test_gpu_hmc_adapt.py,
# the CASES comment): its only window ends at transition 11, so three warm-up transitions and
# the four collected ones run on the new metric.
_WIDE_WARMUP = (0.8, 1, 2, 10, 0.05, 1e-6)  # target_accept, start_buffer, end_buffer, initial_window, regularize, jitter


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("mode", [1, 2], ids=["step_size", "diagonal"])
@pytest.mark.parametrize("shape", [(70, 65), (300, 128)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_hmc_warmup_follows_the_transcription(gm, shape, mode, family):
    """hmc_adapt_kernel<f64, 64, 2, GlmT, 1 and 2> at three and at four column chunks."""
    N, D = shape
    L, eps0, n_collect, n_discard = 4, 0.02, 4, 14
    assert href.window_ends(14, 1, 2, 10) == [11]
    ref, kw, x0 = _wide_hmc_case(gm, N, D, family)
    draws = _engine_draws(gm, N_WIDE_CHAINS, D, _WIDE_HMC_SEED, n_collect + n_discard)
    cfg = gm.HMCAdaptConfig(("none", "step_size", "diagonal")[mode], *_WIDE_WARMUP)
    s = gm.HMC.with_adaptation(gm.GLM(**kw), x0, eps0, L, cfg, dtype=np.float64).set_seed(_WIDE_HMC_SEED)
    assert s.layout() == (64, 2)
    out = s.run(n_collect, n_discard)
    eps, bar = s.step_sizes()
    gpu = dict(q=s.positions(), samples=out, acc=s.accept_counts(), eps=eps, eps_bar=bar, dinv=s.metric()[0])
    s.close()
    r, r2, sens = _hmc_reference(ref, x0, eps0, L, n_collect, n_discard, mode, draws, _WIDE_WARMUP)
    if mode == 1:
        np.testing.assert_array_equal(gpu["dinv"], np.ones_like(gpu["dinv"]))
    else:
        assert np.all(gpu["dinv"] != 1.0)
    _assert_hmc_tie(f"{family} {N}x{D} mode {mode}", gpu, r, r2, sens, mode, n_discard)


# ---- 3b. NUTS follows its transcription ------------------------------------------------
def _nuts_result(s, out):
    eps, bar = s.step_sizes()
    return dict(samples=out, q=s.positions(), eps=eps, eps_bar=bar, acc=s.accept_counts(), nlf=s.leapfrog_counts())


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("metric", ["identity", "diagonal_unit"])
@pytest.mark.parametrize("shape", R.NUTS_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_nuts_follows_the_transcription(gm, oracle, shape, metric, family):
    """nuts_kernel<f64, 64, E, GlmT, MASS, recording> tree by tree against
    tests/_nuts_ref.py with GlmRef.logp_grad, the step size from the sampler's
    own search. "diagonal_unit" is the MASS 1 unit with windows so long that
    none ends within the 9 transitions: the metric stays the identity, and the
    same transcription is the reference (the evaluation is what is specific to
    the GLM in that instantiation; its metric arithmetic is pinned bit for bit
    on the built-in targets, tests/test_gpu_nuts_mass.py). The conditions on
    the transcription are those of tests/test_nuts_ref.py, which checks them
    without a GPU."""
    N, D, layout = shape
    c = R.NUTS_RUN
    ref, kw, x0 = R.nuts_case(N, D, family)
    r, r2, sens = R.nuts_reference(oracle, N, D, family)
    if metric == "identity":
        s = gm.NUTS(gm.GLM(**kw), x0, c["target_accept"], dtype=np.float64, max_depth=c["max_depth"])
    else:
        s = gm.NUTS.new_with_mass_matrix(gm.GLM(**kw), x0, c["target_accept"],
                                         gm.NUTSMassMatrixConfig("diagonal", 50, 50, 10), dtype=np.float64,
                                         max_depth=c["max_depth"])
    s.set_seed(c["seed"])
    assert s.layout() == _default_layout(D)
    if layout is not None:
        s.set_layout(*layout)
    s.collect_stats("all")
    out = s.run(c["n_collect"], c["n_discard"])
    gpu = _nuts_result(s, out)
    st = s.last_stats()
    depth, n_leapfrog = st.tree_depth.astype(np.int64), st.n_leapfrog.astype(np.int64)
    if metric != "identity":
        np.testing.assert_array_equal(s.mass_matrix().kind, 0)
    s.close()
    dev = _nuts_ref.deviation(gpu, r)
    print(f"{family} {N}x{D} {metric}: margin {r['margin'].min():.3e}, leapfrogs {r['nlf']}, depths up to "
          f"{r['depth'].max()}, sensitivity {sens:.3e}, GPU deviation {dev:.3e}, dev / sens {dev / sens:.1e}")
    assert r["margin"].min() >= 1e-9, r["margin"]
    assert _nuts_ref.same_decisions(r, r2)
    assert 0 < sens <= 1e-4, sens
    assert r["depth"].max() >= 3
    np.testing.assert_array_equal(depth, r["depth"])
    np.testing.assert_array_equal(n_leapfrog, r["n_leapfrog"])
    np.testing.assert_array_equal(gpu["nlf"], r["nlf"])
    np.testing.assert_array_equal(gpu["acc"], r["acc"])
    assert dev <= 16 * sens, (dev, sens)


_TAG_NUTS_MOM = 6


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("shape", [(70, 65), (300, 128)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_nuts_variants_give_the_same_bits(gm, oracle, shape, family, dtype):
    """The same samples and step sizes wherever the subtree stack lies (the
    default puts the GLM staging area under up to three stack levels in LDS at
    64 x 2 f64), with the momenta drawn inside the tree kernel, from the
    recording units, and for chain 5 alone.

    The recording run also shows the log-density the kernel carries: a
    transition's recorded energy is K(p0) - logp(q) at its start, the logp
    part reduced together with the kinetic energy (eval_part / finish). For
    the transitions that start at a collected row, q is that row and p0 the
    transition's momentum draw, so logp = K(p0) - energy is checked against
    GlmRef.rounded(dtype) within test 1's bound plus the rounding of the
    kinetic sum and of the difference, (D + 2) u (K + |K - logp|) to first
    order in any summation order."""
    N, D = shape
    n_chains, n_collect, n_discard, seed = 6, 4, 6, 17
    X, y, off = R.synth(N, D, family, 3)
    ref = R.GlmRef(X, y, family, 2.0, off)
    target = gm.GLM(X, y, family=family, prior_sd=2.0, offset=off)
    x0 = (0.3 * gm.init_with_seed(n_chains, D, 14, np.float64)).astype(dtype)

    def run(setup=None, first=0, n=n_chains, stats=False):
        s = gm.NUTS(target, x0[first:first + n], 0.8, dtype=dtype, max_depth=6, chain_offset=first).set_seed(seed)
        assert s.layout() == (64, 2)
        if setup:
            setup(s)
        out = s.run(n_collect, n_discard)
        res = _nuts_result(s, out)
        if stats:
            res["energy"] = s.last_stats().energy.astype(np.float64)
            res["depth"] = s.last_stats().tree_depth
        s.close()
        return res

    base = run()
    assert np.all(np.isfinite(base["samples"])) and base["acc"].min() > 0
    variants = {"lds levels 0": run(lambda s: s.set_lds_levels(0)), "lds levels 1": run(lambda s: s.set_lds_levels(1)),
                "momenta in the tree kernel": run(lambda s: s.set_momentum_pass(False)),
                "recording": run(lambda s: s.collect_stats(True), stats=True)}
    for name, v in variants.items():
        for k in ("samples", "q", "eps", "eps_bar", "acc", "nlf"):
            np.testing.assert_array_equal(v[k], base[k], err_msg=f"{name}: {k}")
    one = run(first=5, n=1)
    for k in ("samples", "q", "eps", "eps_bar", "acc", "nlf"):
        np.testing.assert_array_equal(one[k][0], base[k][5], err_msg=f"chain 5 alone: {k}")

    # the carried log-density: stats column i is the transition that produced row i, which is
    # transition n_discard - 1 + i of the run and starts at row i - 1
    energy = variants["recording"]["energy"]
    assert energy.shape == (n_chains, n_collect)
    assert variants["recording"]["depth"].max() >= 3
    nrm = getattr(oracle.lib, "or_normal_f" if dtype == np.float32 else "or_normal_d")
    u = R.unit_roundoff(dtype)
    rr = ref.rounded(dtype)
    worst = 0.0
    for i in range(1, n_collect):
        q = base["samples"][:, i - 1].astype(np.float64)
        p0 = np.array([[nrm(seed, c, n_discard - 1 + i, _TAG_NUTS_MOM, j) for j in range(D)] for c in range(n_chains)],
                      dtype=np.float64)
        K = 0.5 * np.sum(p0 * p0, axis=1)
        lp_ref, _ = rr.logp_grad(q)
        S, _ = rr.scales(q)
        bound = R.bound(ref, dtype) * S + (D + 2) * u * (K + np.abs(K - lp_ref))
        worst = max(worst, float(np.max(np.abs((K - energy[:, i]) - lp_ref) / bound)))
    print(f"{family} {N}x{D} {np.dtype(dtype).name}: carried |d logp| / bound = {worst:.3e}")
    assert worst <= 1.0


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("case", [(70, 33, (64, 1))], ids=lambda c: f"{c[0]}x{c[1]}")
def test_nuts_f32_against_the_same_model_as_a_custom_target(gm, case, family):
    """The float32 gradient inside NUTS. At test 1's f32 bound a perturbed
    float64 transcription changes its decisions, so no float64 tie covers it;
    instead the GLM sampler is compared with the same model as a
    run-time-compiled CustomTarget (tests/custom_targets.py GLM): the same
    NUTS kernel and the same draws, only the rounding of the evaluation
    differs. The yardstick for that rounding is a second custom source that
    walks the rows in descending order: dev(GLM, A) <= 16 dev(A, B), with
    dev(A, B) > 0 and the same leapfrog counts in all three.

    Two column chunks only: each of the two sources takes about 5 s to compile
    at D = 33 and 23 - 25 s at D = 65 (70 x 65 at 64 x 2 passed the same
    assertions at ratios 3.0 and 0.85 when it was run; DESIGN.md, "GLM
    target"), too long for a test that every later change runs again."""
    N, D, layout = case
    dtype = np.float32
    X, y, off = R.synth(N, D, family, 3)
    x0 = (0.3 * np.random.default_rng(5).standard_normal((4, D))).astype(dtype)
    params = ct.glm_params(X, y, family, 2.0, off)

    def run(target, lay=None):
        t0 = time.perf_counter()
        s = gm.NUTS(target, x0, 0.8, dtype=dtype, max_depth=4).set_seed(17)
        if lay is not None:
            s.set_layout(*lay)
        out = s.run(2, 2)
        dt = time.perf_counter() - t0
        res = _nuts_result(s, out)
        s.close()
        return res, dt

    glm, _ = run(gm.GLM(X, y, family=family, prior_sd=2.0, offset=off), layout)
    a, ta = run(gm.CustomTarget(ct.GLM, D, params))
    b, tb = run(gm.CustomTarget(ct.GLM_ROWS_DESCENDING, D, params))
    dev, yard = _nuts_ref.deviation(glm, a), _nuts_ref.deviation(b, a)
    print(f"{family} {N}x{D}: custom sampler create + compile + run {ta:.1f} s and {tb:.1f} s, leapfrogs {a['nlf']}, "
          f"dev(A, B) {yard:.3e}, dev(GLM, A) {dev:.3e}, ratio {dev / yard if yard else np.inf:.3f}")
    assert np.all(np.isfinite(glm["samples"])) and a["nlf"].min() >= 3
    np.testing.assert_array_equal(glm["nlf"], a["nlf"])
    np.testing.assert_array_equal(b["nlf"], a["nlf"])
    assert yard > 0
    assert dev <= 16 * yard, (dev, yard)


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
