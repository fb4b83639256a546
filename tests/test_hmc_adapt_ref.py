"""The HMC warm-up without a GPU: the numpy transcription of its semantics
(tests/_hmc_adapt_ref.py) meets, on numpy's own draws, the intervals that
tests/test_gpu_hmc_adapt.py asserts of the GPU at the same shape; the window
schedule; and the new ABI symbols and facade names exist."""
import dataclasses

import numpy as np
import pytest

from tests import _hmc_adapt_ref as ref

NEW_SYMBOLS = ["gm_hmc_set_adaptation", "gm_hmc_set_step_sizes", "gm_hmc_get_step_sizes", "gm_hmc_set_metric",
               "gm_hmc_get_metric"]


def test_window_schedule():
    # start 5, end 10, first window 10, 60 warm-up transitions: the windows
    # close at 15, 25, 45 and, with 4 positions only, 49
    assert ref.window_ends(60, 5, 10, 10) == [15, 25, 45, 49]
    assert ref.window_ends(400, 75, 50, 25) == [100, 125, 175, 275, 349]
    assert ref.window_ends(60, 75, 50, 25) == []  # a warm-up shorter than its buffers adapts no metric
    assert ref.window_ends(0, 75, 50, 25) == []


@pytest.mark.parametrize("seed", [0, 1])
def test_transcription_meets_the_statistical_intervals(seed):
    sigma = np.geomspace(0.5, 8.0, 8)
    f = ref.diag_gauss(sigma)
    rng = np.random.default_rng(seed)
    x0 = rng.standard_normal((256, 8))

    def draws(t):
        return rng.standard_normal((256, 8)), rng.random(256)

    r = ref.run(f, x0, 1.0, 10, 200, 400, 0, draws)
    assert r["accept_sampling"] < 0.3
    assert np.all(r["eps"] == 1.0) and np.all(r["dinv"] == 1.0)
    r = ref.run(f, x0, 1.0, 10, 200, 400, 1, draws)
    assert 0.75 <= r["accept_sampling"] <= 0.95
    assert 0.45 <= np.median(r["eps"]) <= 0.8
    assert np.all(r["dinv"] == 1.0) and np.array_equal(r["eps"], r["eps_bar"])
    r = ref.run(f, x0, 1.0, 10, 200, 400, 2, draws)
    assert 0.78 <= r["accept_sampling"] <= 0.98
    ratio = np.median(r["dinv"] / sigma ** 2, axis=0)
    assert np.all((0.7 <= ratio) & (ratio <= 1.4)), ratio
    var = r["samples"].reshape(-1, 8).var(axis=0) / sigma ** 2
    assert np.all((0.85 <= var) & (var <= 1.15)), var
    np.testing.assert_allclose(r["dsq"], 1.0 / np.sqrt(r["dinv"]), rtol=1e-15)


def test_identity_metric_and_fixed_step_leave_the_transition_alone():
    """Mode 0 of the transcription with unit metric is plain HMC: a metric
    dinv = s^2 on a target scaled by s gives s times the plain chain."""
    rng = np.random.default_rng(5)
    s = np.array([1.0, 2.0, 0.25, 8.0])
    sigma = np.array([1.0, 0.5, 2.0, 1.5])
    x0 = rng.standard_normal((7, 4))
    zs, us = rng.standard_normal((12, 7, 4)), rng.random((12, 7))
    a = ref.run(ref.diag_gauss(sigma * s), x0 * s, 0.3, 3, 8, 4, 0, lambda t: (zs[t], us[t]), dinv0=s * s)
    b = ref.run(ref.diag_gauss(sigma), x0, 0.3, 3, 8, 4, 0, lambda t: (zs[t], us[t]))
    np.testing.assert_array_equal(a["accepted"], b["accepted"])
    np.testing.assert_allclose(a["samples"], b["samples"] * s, rtol=1e-12)


def test_new_symbols_are_declared_bound_and_exported():
    import general_mcmc_amd as g
    lib = g._lib.load()
    for n in NEW_SYMBOLS:
        assert n in g._lib.SIGNATURES
        assert hasattr(lib, n)


def test_facade_names_and_defaults():
    import general_mcmc_amd as g
    cfg = g.HMCAdaptConfig()
    mass = g.NUTSMassMatrixConfig()
    assert dataclasses.astuple(cfg) == ("diagonal", 0.8, mass.start_buffer, mass.end_buffer, mass.initial_window,
                                        mass.regularize, mass.jitter) == ("diagonal", 0.8, 75, 50, 25, 0.05, 1e-6)
    assert [g.HMCAdaptConfig(a).mode for a in ("none", "step_size", "diagonal")] == [0, 1, 2]
    for name in ("set_adaptation", "with_adaptation", "step_sizes", "set_step_sizes", "metric", "set_metric"):
        assert callable(getattr(g.HMC, name))
    assert "HMCAdaptConfig" in g.__all__
    assert g.CustomTarget._KINDS["hmc_adapt"] == 4


def test_custom_target_compiles_into_the_warmup_kernel():
    """gm_custom_target_check kind 4: the runtime compiler builds
    hmc_adapt_kernel around a user target (no device needed to compile)."""
    import general_mcmc_amd as g
    from tests import custom_targets as ct
    g.CustomTarget(ct.ISO_GAUSS, 4, [1.0]).check("hmc_adapt", np.float32)
    with pytest.raises(g.GMError, match="undeclared identifier"):
        g.CustomTarget(ct.BROKEN, 4).check("hmc_adapt", np.float64)
