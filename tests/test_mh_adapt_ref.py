"""The MH warm-up without a GPU: the numpy transcription of its semantics
(tests/_mh_adapt_ref.py) meets, on numpy's own draws, the intervals that
tests/test_gpu_mh_adapt.py asserts of the GPU at the same shape; a
power-of-two shape is an exact reparametrisation; the window schedule at the
MH defaults; and the new ABI symbols and facade names exist.

Each interval below is followed by the value the transcription gave over
seeds 0..3 and both starts (proposal_std 8 and 0.01); the intervals are about
ten seed-spreads wide."""
import dataclasses

import numpy as np
import pytest

from tests import _mh_adapt_ref as ref

NEW_SYMBOLS = ["gm_mh_set_adaptation", "gm_mh_set_proposal_scales", "gm_mh_get_proposal_scales",
               "gm_mh_set_proposal_diag", "gm_mh_get_proposal_diag"]

SIGMA, N_CHAINS, N_COLLECT, N_DISCARD = ref.SIGMA, ref.N_CHAINS, ref.N_COLLECT, ref.N_DISCARD
check_control, check_mode1, check_mode2 = ref.check_control, ref.check_mode1, ref.check_mode2


def test_window_schedule_at_the_mh_defaults():
    assert ref.window_ends(1000, 75, 150, 25) == [100, 125, 175, 275, 475, 849]
    assert ref.window_ends(60, 5, 10, 10) == [15, 25, 45, 49]
    assert ref.window_ends(200, 75, 150, 25) == []  # a warm-up shorter than its buffers adapts no shape


@pytest.mark.parametrize("seed", [0, 1])
def test_transcription_meets_the_statistical_intervals(seed):
    f = ref.diag_gauss_logp(SIGMA)
    rng = np.random.default_rng(seed)
    x0 = rng.standard_normal((N_CHAINS, 8))

    def draws(t):
        return rng.standard_normal((N_CHAINS, 8)), rng.random(N_CHAINS)

    r = ref.run(f, x0, 8.0, N_COLLECT, N_DISCARD, 0, draws)
    check_control(r["accept_sampling"])
    assert np.all(r["scale"] == 8.0) and np.all(r["diag"] == 1.0)
    for start in (8.0, 0.01):
        r = ref.run(f, x0, start, N_COLLECT, N_DISCARD, 1, draws)
        print(f"start {start} mode 1: accept {r['accept_sampling']:.3f}, median scale {np.median(r['scale']):.3f}, "
              f"lag-1 {ref.lag1_autocorr(r['samples'], 7):.4f}")
        check_mode1(r["accept_sampling"], r["scale"], r["scale_bar"], r["diag"], r["samples"])
        r = ref.run(f, x0, start, N_COLLECT, N_DISCARD, 2, draws)
        print(f"start {start} mode 2: accept {r['accept_sampling']:.3f}, diag/sigma "
              f"{np.median(r['diag'] / SIGMA, axis=0)}, lag-1 {ref.lag1_autocorr(r['samples'], 7):.4f}")
        check_mode2(r["accept_sampling"], r["scale"], r["scale_bar"], r["diag"], r["samples"])


def test_power_of_two_shape_is_an_exact_reparametrisation():
    """A shape diag = s (powers of two) on a target scaled by s gives s times
    the plain chain, bit for bit: every difference is a scaling by a power of
    two."""
    rng = np.random.default_rng(5)
    s = np.array([1.0, 2.0, 0.25, 8.0])
    sigma = np.array([1.0, 0.5, 2.0, 1.5])
    x0 = rng.standard_normal((7, 4))
    zs, us = rng.standard_normal((40, 7, 4)), rng.random((40, 7))
    a = ref.run(ref.diag_gauss_logp(sigma * s), x0 * s, 0.5, 30, 10, 0, lambda t: (zs[t], us[t]), diag0=s)
    b = ref.run(ref.diag_gauss_logp(sigma), x0, 0.5, 30, 10, 0, lambda t: (zs[t], us[t]))
    np.testing.assert_array_equal(a["accepted"], b["accepted"])
    np.testing.assert_array_equal(a["samples"], b["samples"] * s)
    assert 0 < a["accepted"].sum() < a["accepted"].size


def test_new_symbols_are_declared_bound_and_exported():
    import os

    import general_mcmc_amd as g
    lib = g._lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "gmcmc.h")).read()
    for n in NEW_SYMBOLS:
        assert f"int {n}(gm_sampler*" in header
        assert n in g._lib.SIGNATURES
        assert hasattr(lib, n)


def test_facade_names_and_defaults():
    import general_mcmc_amd as g
    cfg = g.MHAdaptConfig()
    assert dataclasses.astuple(cfg) == ("diagonal", 0.234, 75, 150, 25, 0.05, 1e-6)
    assert [g.MHAdaptConfig(a).mode for a in ("none", "scale", "diagonal")] == [0, 1, 2]
    with pytest.raises(ValueError):
        g.MHAdaptConfig("dense").mode
    for name in ("set_adaptation", "with_adaptation", "proposal_scales", "set_proposal_scales", "proposal_diag",
                 "set_proposal_diag"):
        assert callable(getattr(g.MetropolisHastings, name))
    assert "MHAdaptConfig" in g.__all__
    assert g.CustomTarget._KINDS["mh_adapt"] == 6


def test_custom_target_compiles_into_the_warmup_kernel():
    """gm_custom_target_check kind 6: the runtime compiler builds
    mh_adapt_kernel around a user target (no device needed to compile)."""
    import general_mcmc_amd as g
    from tests import custom_targets as ct
    g.CustomTarget(ct.ISO_GAUSS, 4, [1.0]).check("mh_adapt", np.float32)
    g.CustomTarget(ct.ISO_GAUSS, 4, [1.0]).check("mh_adapt", np.float64)
    with pytest.raises(g.GMError, match="undeclared identifier"):
        g.CustomTarget(ct.BROKEN, 4).check("mh_adapt", np.float64)
