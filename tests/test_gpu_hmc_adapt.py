"""HMC warm-up on the GPU: per-chain step sizes, a per-chain diagonal metric
and their adaptation (gm_hmc_set_adaptation / gm_hmc_set_step_sizes /
gm_hmc_set_metric; hmc_adapt_kernel).

1. equal step sizes + identity metric give the plain kernel's bits;
2. chain c with its own step size is the one-chain plain sampler of that size;
3. a power-of-two metric is an exact reparametrisation of the target;
4. the adaptation recurrences follow the numpy float64 transcription
   (tests/_hmc_adapt_ref.py) driven by the engine's own draws;
5. a warmed-up sampler resumes from a checkpoint bit for bit;
6. user targets (runtime-compiled) take the same path;
7. on a badly scaled Gaussian the warm-up does what it is for;
8. the error paths.
"""
import ctypes as C

import numpy as np
import pytest

from tests import _hmc_adapt_ref as ref
from tests import custom_targets as ct

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


def _prec_gauss(gm, mean, prec):
    """A Gaussian target given by its precision matrix as it stands (no
    inversion: the entries reach the device exactly), norm_const 0."""
    from general_mcmc_amd import _lib

    class PrecGauss(gm.distributions._TargetBase):
        def __init__(self):
            self.mean = np.ascontiguousarray(mean, dtype=np.float64)
            self.prec = np.ascontiguousarray(prec, dtype=np.float64)
            self.dim = self.mean.shape[0]

        def _fill(self, t, dim):
            t.kind = _lib.GM_TARGET_GAUSS
            t.mean = self.mean.ctypes.data_as(C.POINTER(C.c_double))
            t.prec = self.prec.ctypes.data_as(C.POINTER(C.c_double))
            t.norm_const = 0.0
            return [self.mean, self.prec]

    return PrecGauss()


def _target(gm, name, dim):
    if name == "rosenbrock":
        return gm.RosenbrockND(), 0.01
    if name == "iso":
        return gm.IsotropicGaussian(1.3), 0.2
    rng = np.random.default_rng(dim)
    a = rng.standard_normal((dim, dim))
    return gm.DenseGaussian(rng.standard_normal(dim), a @ a.T / dim + np.eye(dim)), 0.15


def _same_run(a, b, n_collect, n_discard):
    np.testing.assert_array_equal(a.run(n_collect, n_discard), b.run(n_collect, n_discard))
    np.testing.assert_array_equal(a.positions(), b.positions())
    np.testing.assert_array_equal(a.accept_counts(), b.accept_counts())


# ---- 1. equal step sizes, identity metric == the plain kernel ----------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["rosenbrock", "iso", "gauss"])
@pytest.mark.parametrize("dim", [1, 3, 64, 65, 200])
def test_equal_step_sizes_are_the_plain_kernel(gm, dtype, name, dim):
    n_chains = 70
    target, eps = _target(gm, name, dim)
    x0 = (gm.init_with_seed(n_chains, dim, 11, np.float64) * 0.5).astype(dtype)
    for n_leapfrog in (1, 2, 7):
        for unroll in (1, 2, 4):
            pair = []
            for adaptive in (False, True):
                s = gm.HMC(target, x0, eps, n_leapfrog, dtype=dtype, chain_offset=5).set_seed(3)
                s.set_steps_per_launch(3).set_unroll(unroll)
                if adaptive:
                    s.set_step_sizes(np.full(n_chains, eps))
                pair.append(s)
            _same_run(pair[0], pair[1], 7, 5)
            for s in pair:
                s.close()


# ---- 2. per-chain step sizes -------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", [3, 65])
def test_per_chain_step_size_is_that_chains_plain_sampler(gm, dtype, dim):
    n_chains, eps, n_leapfrog = 9, 0.01, 5
    x0 = (gm.init_with_seed(n_chains, dim, 12, np.float64) * 0.5).astype(dtype)
    epsc = eps * (1.0 + np.arange(n_chains) / 8.0)
    s = gm.HMC(gm.RosenbrockND(), x0, eps, n_leapfrog, dtype=dtype).set_seed(8).set_step_sizes(epsc)
    out = s.run(6, 3)
    np.testing.assert_array_equal(s.step_sizes()[0], epsc.astype(dtype).astype(np.float64))
    for c in range(n_chains):
        one = gm.HMC(gm.RosenbrockND(), x0[c:c + 1], float(epsc[c]), n_leapfrog, dtype=dtype,
                     chain_offset=c).set_seed(8)
        np.testing.assert_array_equal(one.run(6, 3)[0], out[c])
        np.testing.assert_array_equal(one.positions()[0], s.positions()[c])
        assert one.accept_counts()[0] == s.accept_counts()[c]
        one.close()


# ---- 3. the metric as an exact reparametrisation -----------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_power_of_two_metric_is_an_exact_reparametrisation(gm, dtype):
    """Sampler A: target (mu, P) with M^-1 = s^2. Sampler B, plain: target
    (mu/s, diag(s) P diag(s)) from x/s. Every difference between the two is a
    scaling by a power of two, so A's samples are s * B's bit for bit."""
    n_chains, dim = 33, 5
    s_ = np.array([1.0, 2.0, 0.25, 8.0, 0.5])
    mu = np.array([0.5, -1.0, 0.25, 2.0, -0.75])
    prec = 2.0 * np.eye(dim) - 0.5 * (np.eye(dim, k=1) + np.eye(dim, k=-1)) + 0.25 * (
        np.eye(dim, k=2) + np.eye(dim, k=-2))
    x = gm.init_with_seed(n_chains, dim, 13, np.float64).astype(dtype)
    a = gm.HMC(_prec_gauss(gm, mu, prec), x, 0.125, 5, dtype=dtype).set_seed(4).set_metric(s_ * s_)
    b = gm.HMC(_prec_gauss(gm, mu / s_, prec * np.outer(s_, s_)), (x / s_.astype(dtype)).astype(dtype), 0.125, 5,
               dtype=dtype).set_seed(4)
    dinv, dsq = a.metric()
    np.testing.assert_array_equal(dinv, np.broadcast_to((s_ * s_).astype(dtype), (n_chains, dim)))
    np.testing.assert_array_equal(dsq, np.broadcast_to((1.0 / s_).astype(dtype), (n_chains, dim)))
    np.testing.assert_array_equal(a.run(8, 4), b.run(8, 4) * s_.astype(dtype))
    np.testing.assert_array_equal(a.accept_counts(), b.accept_counts())
    assert 0 < a.accept_counts().sum() < 12 * n_chains  # both branches of the accept were taken


# ---- 4. the recurrences against the numpy transcription -----------------------
# The GPU's largest deviation from the float64 transcription, measured on an
# MI355X (eps, eps_bar, dinv, dsq relative; positions and samples relative to
# the coordinate's sigma); the assertion allows 64 times that. The first two
# cases are far above float64 rounding, and that is a property of the
# recurrence at this shape, not of the kernel: the warm-up starts from
# mu = ln(10 * 0.5) on a target whose smallest sigma is 0.5, so its first
# transitions integrate with eps*omega > 2, where the leapfrog map expands
# differences exponentially, and the dual averaging feeds them back into eps.
# The transcription itself, with x0 moved by one ulp, ends 4e-8 (this seed,
# the calmest of seeds 1..40 under the CPU oracle's draws) to 1e-3 away from
# its own unperturbed run; the kernel differs from it by an ulp in every fused
# multiply-add and reduction. The third case stops 11 transitions after the
# first window end, before most of that growth, and pins the window-end
# arithmetic (metric, restart) much more tightly. DESIGN.md, "HMC warm-up".
CASES = {
    # name: (mode, n_collect, n_discard, measured deviation)
    "step_size": (1, 20, 60, 9.1e-9),     # eps 7.9e-10, q 3.6e-9, samples 9.0e-9
    "diagonal": (2, 20, 60, 2.5e-3),      # eps 6.3e-5, dinv 2.1e-8, q 1.1e-3, samples 2.5e-3
    "first_window": (2, 0, 26, 9.1e-11),  # eps 4.3e-12, dinv 5.8e-14, q 9.1e-11
}
_SIGMA4 = np.array([0.5, 1.0, 3.0])


def _engine_draws(gm, n_chains, dim, seed, n):
    from general_mcmc_amd import batch_vector as bv
    z = bv.DeviceMatrix((n_chains, dim), np.float64)
    zs, us = [], []
    for t in range(n):
        bv.fill_random_normal(z, seed, t)
        zs.append(z.to_host())
        us.append(bv.sample_uniform(n_chains, np.float64, seed, t).to_host())
    return lambda t: (zs[t], us[t])


@pytest.fixture(scope="module")
def recurrences(gm):
    """(GPU results, transcription) per case, the transcription driven by the
    engine's own momentum normals and accept uniforms."""
    n_chains, dim, n_leapfrog, eps0, seed = 6, 3, 4, 0.5, 29
    x0 = gm.init_with_seed(n_chains, dim, 14, np.float64)
    prec = 1.0 / _SIGMA4 ** 2
    draws = _engine_draws(gm, n_chains, dim, seed, 80)

    def logp_grad(q):
        return -0.5 * np.sum(q * q * prec, axis=1), -q * prec

    res = {}
    for case, (mode, n_collect, n_discard, _) in CASES.items():
        s = gm.HMC(_prec_gauss(gm, np.zeros(dim), np.diag(prec)), x0, eps0, n_leapfrog, dtype=np.float64)
        s.set_seed(seed).set_adaptation(gm.HMCAdaptConfig(("none", "step_size", "diagonal")[mode], 0.8, 5, 10, 10,
                                                          0.05, 1e-6))
        out = s.run(n_collect, n_discard)
        eps, bar = s.step_sizes()
        dinv, dsq = s.metric()
        gpu = dict(eps=eps, eps_bar=bar, dinv=dinv, dsq=dsq, q=s.positions(), samples=out, acc=s.accept_counts())
        r = ref.run(logp_grad, x0, eps0, n_leapfrog, n_collect, n_discard, mode, draws, 0.8, 5, 10, 10, 0.05, 1e-6)
        res[case] = (gpu, r)
        s.close()
    return res


def _deviation(gpu, r):
    dev = {k: float(np.max(np.abs(gpu[k] - r[k]) / np.abs(r[k]))) for k in ("eps", "eps_bar", "dinv", "dsq")}
    dev["q"] = float(np.max(np.abs(gpu["q"] - r["q"]) / _SIGMA4))
    if r["samples"].size:
        dev["samples"] = float(np.max(np.abs(gpu["samples"] - r["samples"]) / _SIGMA4))
    return dev


@pytest.mark.parametrize("case", list(CASES))
def test_recurrences_follow_the_transcription(recurrences, case):
    mode, n_collect, n_discard, measured = CASES[case]
    assert ref.window_ends(60, 5, 10, 10) == [15, 25, 45, 49]  # the last one has 4 positions: no update
    assert ref.window_ends(26, 5, 10, 10) == [15]
    gpu, r = recurrences[case]
    # no accept decision of the transcription is within rounding of its threshold
    assert r["margin"] >= 1e-9, r["margin"]
    dev = _deviation(gpu, r)
    print(f"{case}: deviation from the transcription {dev}, decision margin {r['margin']:.3e}")
    # the decisions agree on every (chain, transition): equal totals per chain,
    # equal moves in the collected rows and, through the positions, equal paths
    np.testing.assert_array_equal(gpu["acc"], r["accepted"].sum(axis=0))
    if n_collect:
        moved = np.any(gpu["samples"][:, 1:] != gpu["samples"][:, :-1], axis=2)
        np.testing.assert_array_equal(moved, r["accepted"][n_discard + 1:].T)
    if mode == 1:
        np.testing.assert_array_equal(gpu["dinv"], np.ones_like(gpu["dinv"]))
    else:
        assert np.all(gpu["dinv"] != 1.0)
    assert max(dev.values()) <= 64 * measured, dev


# ---- 5. checkpoint ---------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_warmed_up_sampler_resumes_bit_for_bit(gm, dtype):
    n_chains, dim = 40, 5
    x0 = gm.init_with_seed(n_chains, dim, 15, np.float64).astype(dtype)
    target = _prec_gauss(gm, np.zeros(dim), np.diag(1.0 / np.array([0.5, 1.0, 2.0, 4.0, 8.0]) ** 2))
    cfg = gm.HMCAdaptConfig("diagonal", 0.8, 5, 10, 10, 0.05, 1e-6)
    a = gm.HMC(target, x0, 0.5, 4, dtype=dtype).set_seed(6)
    plain_blob = a.save_state()
    a.set_adaptation(cfg)
    a.run(0, 60)
    blob = a.save_state()
    assert len(blob) > len(plain_blob)
    b = gm.HMC(target, x0, 0.5, 4, dtype=dtype).load_state(blob)
    for x, y in zip(a.step_sizes() + a.metric(), b.step_sizes() + b.metric()):
        np.testing.assert_array_equal(x, y)
    assert np.all(a.metric()[0] != 1.0) and np.all(a.step_sizes()[0] != 0.5)
    _same_run(a, b, 10, 0)
    for x, y in zip(a.step_sizes() + a.metric(), b.step_sizes() + b.metric()):
        np.testing.assert_array_equal(x, y)
    assert b.save_state() == a.save_state()
    # mode 0 drops the per-chain state: the blob is a plain sampler's again, and
    # a plain blob loaded into an adaptive sampler returns it to the plain path
    a.set_adaptation(gm.HMCAdaptConfig("none"))
    assert len(a.save_state()) == len(plain_blob)
    b.load_state(plain_blob)
    assert b.save_state() == plain_blob
    np.testing.assert_array_equal(b.step_sizes()[0], np.full(n_chains, float(dtype(0.5))))


@pytest.mark.parametrize("dtype", DTYPES)
def test_checkpoint_mid_warmup_configuration(gm, dtype):
    """An armed sampler saved before its warm-up runs it after the load."""
    x0 = gm.init_with_seed(12, 3, 16, np.float64).astype(dtype)
    cfg = gm.HMCAdaptConfig("diagonal", 0.7, 5, 10, 10, 0.05, 1e-6)
    a = gm.HMC(gm.IsotropicGaussian(2.0), x0, 0.3, 3, dtype=dtype).set_seed(2).set_adaptation(cfg)
    b = gm.HMC(gm.IsotropicGaussian(2.0), x0, 0.3, 3, dtype=dtype).load_state(a.save_state())
    _same_run(a, b, 5, 60)
    for x, y in zip(a.step_sizes() + a.metric(), b.step_sizes() + b.metric()):
        np.testing.assert_array_equal(x, y)
    assert np.all(a.metric()[0] != 1.0)


# ---- run-call behaviour ------------------------------------------------------
def test_arming_and_the_run_calls(gm):
    n_chains, dim = 20, 4
    x0 = gm.init_with_seed(n_chains, dim, 17, np.float64)
    cfg = gm.HMCAdaptConfig("step_size", 0.8)
    s = gm.HMC(gm.IsotropicGaussian(1.5), x0, 0.2, 5).set_seed(1)
    np.testing.assert_array_equal(s.step_sizes()[0], np.full(n_chains, 0.2))
    np.testing.assert_array_equal(s.metric()[0], np.ones((n_chains, dim)))
    s.set_adaptation(cfg)
    s.run(3, 0)  # n_discard == 0: adapts nothing, stays armed
    s.step()     # a step never starts a warm-up
    np.testing.assert_array_equal(s.step_sizes()[0], np.full(n_chains, 0.2))
    s.run(2, 30)
    eps, bar = s.step_sizes()
    assert np.all(eps != 0.2) and np.all(eps > 0) and np.array_equal(eps, bar)  # frozen at eps_bar
    s.run(4, 10)  # not armed any more: the discarded transitions are plain burn-in
    s.step()
    np.testing.assert_array_equal(s.step_sizes()[0], eps)
    assert np.all(s.leapfrog_counts() == (3 + 1 + 32 + 14 + 1) * 5)
    s.set_adaptation(cfg)  # re-armed: starts from the current step sizes
    s.run(0, 25)
    assert np.all(s.step_sizes()[0] != eps)
    # mode 0: back on the creation step size and the plain kernel
    s.set_adaptation(gm.HMCAdaptConfig("none"))
    np.testing.assert_array_equal(s.step_sizes()[0], np.full(n_chains, 0.2))
    p = gm.HMC(gm.IsotropicGaussian(1.5), s.positions(), 0.2, 5).set_seed(9)
    s.set_seed(9)
    np.testing.assert_array_equal(s.run(5, 2), p.run(5, 2))


@pytest.mark.parametrize("dtype", DTYPES)
def test_progress_and_async_runs_match_run(gm, dtype):
    n_chains, dim = 50, 6
    x0 = gm.init_with_seed(n_chains, dim, 18, np.float64).astype(dtype)
    cfg = gm.HMCAdaptConfig("diagonal", 0.8, 5, 10, 10, 0.05, 1e-6)

    def make():
        return gm.HMC(gm.IsotropicGaussian(3.0), x0, 0.4, 4, dtype=dtype).set_seed(5).set_adaptation(cfg)

    a, b, c = make(), make(), make()
    out = a.run(10, 60)
    seen = []
    out_b, stats = b.run_progress(10, 60, progress=seen.append, interval=0.0)
    np.testing.assert_array_equal(out, out_b)
    assert stats is not None and seen and seen[-1].done == 10
    c.set_async(True).set_steps_per_launch(7)
    dev = c.run_positions(10, 60)
    c.synchronize()
    np.testing.assert_array_equal(out, dev.to_host())
    for s in (b, c):
        for x, y in zip(a.step_sizes() + a.metric(), s.step_sizes() + s.metric()):
            np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(a.accept_counts(), s.accept_counts())


# ---- 6. user targets ---------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_custom_target(gm, dtype):
    dim, n_chains = 3, 70
    x0 = (gm.init_with_seed(n_chains, dim, 19, np.float64) * 0.5).astype(dtype)
    t = gm.CustomTarget(ct.ROSENBROCK, dim, [1.0, 100.0])
    t.check("hmc_adapt", dtype)
    pair = []
    for adaptive in (False, True):
        s = gm.HMC(t, x0, 0.01, 7, dtype=dtype, chain_offset=5).set_seed(3).set_steps_per_launch(3)
        if adaptive:
            s.set_step_sizes(np.full(n_chains, 0.01))
        pair.append(s)
    _same_run(pair[0], pair[1], 7, 5)
    s = pair[1].set_adaptation(gm.HMCAdaptConfig("diagonal", 0.8, 5, 10, 10, 0.05, 1e-6))
    out = s.run(5, 60)
    eps, bar = s.step_sizes()
    dinv, dsq = s.metric()
    assert np.all(np.isfinite(out))
    assert np.all(np.isfinite(eps)) and np.all(eps > 0) and np.all(eps != 0.01)
    assert np.all(np.isfinite(dinv)) and np.all(dinv > 0) and np.all(dinv != 1.0)
    np.testing.assert_allclose(dsq, 1.0 / np.sqrt(dinv), rtol=1e-6)


# ---- 7. statistical ----------------------------------------------------------
_SIGMA7 = np.geomspace(0.5, 8.0, 8)


def _moves(samples):
    """Acceptance of the collected transitions: the share of consecutive rows
    that differ (an accepted proposal moves every coordinate)."""
    return float(np.mean(np.any(samples[:, 1:] != samples[:, :-1], axis=2)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_warmup_on_a_badly_scaled_gaussian(gm, dtype):
    n_chains, dim = 256, 8
    x0 = gm.init_with_seed(n_chains, dim, 20, np.float64).astype(dtype)
    target = _prec_gauss(gm, np.zeros(dim), np.diag(1.0 / _SIGMA7 ** 2))
    # control: no adaptation
    s = gm.HMC(target, x0, 1.0, 10, dtype=dtype).set_seed(31)
    acc = _moves(s.run(200, 400))
    print(f"control acceptance {acc:.3f}")
    assert acc < 0.3
    # mode 1
    s = gm.HMC.with_adaptation(target, x0, 1.0, 10, gm.HMCAdaptConfig("step_size"), dtype=dtype).set_seed(31)
    acc = _moves(s.run(200, 400))
    med = float(np.median(s.step_sizes()[0]))
    print(f"mode 1 acceptance {acc:.3f}, median eps {med:.3f}")
    assert 0.75 <= acc <= 0.95
    assert 0.45 <= med <= 0.8
    # mode 2
    s = gm.HMC.with_adaptation(target, x0, 1.0, 10, gm.HMCAdaptConfig(), dtype=dtype).set_seed(31)
    out = s.run(200, 400).astype(np.float64)
    acc = _moves(out)
    ratio = np.median(s.metric()[0].astype(np.float64) / _SIGMA7 ** 2, axis=0)
    var = out.reshape(-1, dim).var(axis=0) / _SIGMA7 ** 2
    print(f"mode 2 acceptance {acc:.3f}, median dinv/sigma^2 {ratio}, pooled variance/sigma^2 {var}")
    assert 0.78 <= acc <= 0.98
    assert np.all((0.7 <= ratio) & (ratio <= 1.4))
    assert np.all((0.85 <= var) & (var <= 1.15))


# ---- 8. error paths ----------------------------------------------------------
def _new_calls(gm, s):
    """Return codes of the five new entry points with valid arguments."""
    lib = gm._lib.load()
    n, d = s.n_chains, s.dim
    eps = np.full(n, 0.1)
    m = np.ones((n, d), dtype=s.dtype)
    out1, out2 = np.empty(n), np.empty(n)
    return [lib.gm_hmc_set_adaptation(s._h, 1, 0.8, 75, 50, 25, 0.05, 1e-6),
            lib.gm_hmc_set_step_sizes(s._h, gm._lib.ptr(eps)),
            lib.gm_hmc_get_step_sizes(s._h, gm._lib.ptr(out1), gm._lib.ptr(out2)),
            lib.gm_hmc_set_metric(s._h, gm._lib.ptr(m)),
            lib.gm_hmc_get_metric(s._h, gm._lib.ptr(m), None)]


def test_error_paths(gm):
    L = gm._lib
    x0 = gm.init_det(4, 3)
    mh = gm.MetropolisHastings(gm.IsotropicGaussian(1.0), gm.IsotropicGaussian(0.5), x0)
    nuts = gm.NUTS(gm.IsotropicGaussian(1.0), x0, 0.8)
    assert _new_calls(gm, mh) == [L.GM_ESTATE] * 5
    assert _new_calls(gm, nuts) == [L.GM_ESTATE] * 5
    wide = gm.HMC(gm.RosenbrockND(), gm.init_det(2, 2000, np.float32) * np.float32(0.1), 0.001, 2)
    assert _new_calls(gm, wide) == [L.GM_EINVAL] * 5
    assert b"wide" in L.load().gm_last_error()
    np.testing.assert_array_equal(wide.run(2, 1).shape, (2, 2, 2000))  # and it still runs its own path

    s = gm.HMC(gm.IsotropicGaussian(1.0), x0, 0.1, 3).set_seed(1)
    blob = s.save_state()
    lib = L.load()
    for bad in (0.0, 1.0, float("nan"), -0.2, 1.5):
        assert lib.gm_hmc_set_adaptation(s._h, 1, bad, 75, 50, 25, 0.05, 1e-6) == L.GM_EINVAL
    assert lib.gm_hmc_set_adaptation(s._h, 3, 0.8, 75, 50, 25, 0.05, 1e-6) == L.GM_EINVAL
    assert lib.gm_hmc_set_adaptation(s._h, 2, 0.8, -1, 50, 25, 0.05, 1e-6) == L.GM_EINVAL
    assert lib.gm_hmc_set_adaptation(s._h, 2, 0.8, 75, 50, 25, 1.5, 1e-6) == L.GM_EINVAL
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        m = np.ones((4, 3))
        m[2, 1] = bad
        assert lib.gm_hmc_set_metric(s._h, L.ptr(m)) == L.GM_EINVAL
        e = np.full(4, 0.1)
        e[3] = bad
        assert lib.gm_hmc_set_step_sizes(s._h, L.ptr(e)) == L.GM_EINVAL
    # nothing changed: still the plain sampler, byte for byte
    assert s.save_state() == blob
    np.testing.assert_array_equal(s.metric()[0], np.ones((4, 3)))
    np.testing.assert_array_equal(s.metric()[1], np.ones((4, 3)))
    # a rejected metric leaves a set one in place
    good = np.full((4, 3), 4.0)
    s.set_metric(good)
    m = good.copy()
    m[0, 0] = -1.0
    assert lib.gm_hmc_set_metric(s._h, L.ptr(m)) == L.GM_EINVAL
    np.testing.assert_array_equal(s.metric()[0], good)
    np.testing.assert_array_equal(s.metric()[1], np.full((4, 3), 0.5))
