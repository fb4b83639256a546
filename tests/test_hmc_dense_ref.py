"""The HMC dense metric without a GPU: the numpy transcription of its semantics
(tests/_hmc_dense_ref.py) reduces to the diagonal warm-up's transcription,
its pooled covariance is numpy's, and on cfg3's target (32-D, eigenvalues
0.1 ... 10, random rotation) it recovers the covariance and lets the step size
grow; the new ABI symbols and facade names exist."""
import numpy as np
import pytest

import bench
from tests import _hmc_adapt_ref as dref
from tests import _hmc_dense_ref as ref

NEW_SYMBOLS = ["gm_hmc_set_dense_adaptation", "gm_hmc_set_dense_metric", "gm_hmc_get_dense_metric"]


def gauss(cov):
    prec = np.linalg.inv(cov)
    prec = 0.5 * (prec + prec.T)

    def f(q):
        w = q @ prec
        return -0.5 * np.sum(w * q, axis=1), -w
    return f


def test_identity_metric_without_a_window_is_the_step_size_warmup():
    rng = np.random.default_rng(3)
    sigma = np.array([0.5, 1.0, 3.0, 1.5])
    f = dref.diag_gauss(sigma)
    x0 = rng.standard_normal((9, 4))
    zs, us = rng.standard_normal((50, 9, 4)), rng.random((50, 9))
    draws = lambda t: (zs[t], us[t])  # noqa: E731
    # 30 warm-up transitions end inside the start buffer: no window, the metric stays the identity
    a = ref.run(f, x0, 0.5, 4, 20, 30, True, draws, start_buffer=75)
    b = dref.run(f, x0, 0.5, 4, 20, 30, 1, draws)
    assert a["updates"] == 0 and np.array_equal(a["minv"], np.eye(4))
    np.testing.assert_array_equal(a["accepted"], b["accepted"])
    np.testing.assert_allclose(a["eps"], b["eps"], rtol=1e-13)
    np.testing.assert_allclose(a["samples"], b["samples"], rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("mean", [0.0, 1e4])
def test_pooled_covariance_is_numpys(mean):
    rng = np.random.default_rng(7)
    l = rng.standard_normal((5, 5))
    rows = [mean + rng.standard_normal((70, 5)) @ l.T for _ in range(9)]
    st = ref.Pooled(5)
    for r in rows:
        st.add(r)
    assert st.rn == 9
    np.testing.assert_allclose(st.covariance(), np.cov(np.concatenate(rows), rowvar=False), rtol=1e-9, atol=0)


def test_factor():
    rng = np.random.default_rng(1)
    m = rng.standard_normal((6, 6))
    sig = m @ m.T + np.eye(6)
    a = ref.factor(sig)
    assert np.all(np.tril(a, -1) == 0)
    np.testing.assert_allclose(a @ a.T, np.linalg.inv(sig), rtol=1e-10, atol=1e-12)  # p = A z ~ N(0, Sigma^-1)
    assert ref.factor(np.array([[1.0, 2.0], [2.0, 1.0]])) is None


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_transcription_on_the_rotated_gaussian(seed):
    _, cov = bench.dense_gauss_32()
    f = gauss(cov)
    rng = np.random.default_rng(seed)
    x0 = rng.standard_normal((256, 32))

    def draws(t):
        return rng.standard_normal((256, 32)), rng.random(256)

    r = ref.run(f, x0, 0.5, 3, 200, 400, True, draws)
    assert r["failed"] == 0 and r["updates"] >= 3
    ev = np.linalg.eigvals(np.linalg.solve(cov, r["minv"])).real
    assert 0.7 <= ev.min() and ev.max() <= 1.7, (ev.min(), ev.max())
    d = dref.run(f, x0, 0.5, 3, 200, 400, 2, draws)
    assert np.median(r["eps_bar"]) >= 1.5 * np.median(d["eps_bar"]), (np.median(r["eps_bar"]),
                                                                       np.median(d["eps_bar"]))


def test_new_symbols_are_declared_bound_and_exported():
    import general_mcmc_amd as g
    lib = g._lib.load()
    for n in NEW_SYMBOLS:
        assert n in g._lib.SIGNATURES
        assert hasattr(lib, n)


def test_facade_names():
    import general_mcmc_amd as g
    assert g.HMCAdaptConfig("dense").adaptation == "dense"
    for name in ("dense_metric", "set_dense_metric", "dense_metric_updates"):
        assert callable(getattr(g.HMC, name))


def test_custom_target_compiles_into_the_dense_kernel():
    """gm_custom_target_check kind 5: the runtime compiler builds
    hmc_dense_kernel around a user target at layout (1, dim), smallest and
    largest dim (no device needed to compile); dims outside 2..64 are refused."""
    import general_mcmc_amd as g
    from tests import custom_targets as ct
    assert g.CustomTarget._KINDS["hmc_dense"] == 5
    g.CustomTarget(ct.ISO_GAUSS, 2, [1.0]).check("hmc_dense", np.float32)
    g.CustomTarget(ct.ISO_GAUSS, 5, [1.0]).check("hmc_dense", np.float64)
    for dim in (1, 65):
        with pytest.raises(g.GMError, match="2 <= dim <= 64"):
            g.CustomTarget(ct.ISO_GAUSS, dim, [1.0]).check("hmc_dense", np.float64)
    with pytest.raises(g.GMError, match="undeclared identifier"):
        g.CustomTarget(ct.BROKEN, 4).check("hmc_dense", np.float64)


def test_adapt_config_mode_names_its_error():
    import general_mcmc_amd as g
    for name in ("dense", "nonsense"):
        with pytest.raises(ValueError, match="adaptation"):
            g.HMCAdaptConfig(name).mode
