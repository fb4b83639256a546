"""Per-transition sampler statistics, the parts that need no device: the
transcription the GPU tests compare against, the new C-ABI symbols and the
error paths of gm_sampler_set_stats and the getters."""
import ctypes as C

import numpy as np
import pytest

from tests import _hmc_adapt_ref as ref
from tests import _hmc_stats_ref as sref

NEW_SYMBOLS = ["gm_sampler_set_stats", "gm_sampler_stats_info", "gm_sampler_stats_device",
               "gm_sampler_stats_field", "gm_sampler_stats_reduce", "gm_stats_reduce_device"]


@pytest.mark.parametrize("mode", [0, 1])
def test_statistics_transcription_is_the_warmup_transcription(mode):
    """_hmc_stats_ref.run walks _hmc_adapt_ref.run's path bit for bit, and its
    records are consistent with that path."""
    rng = np.random.default_rng(3)
    sigma = np.array([0.5, 1.0, 3.0])
    x0 = rng.standard_normal((6, 3))
    zs, us = rng.standard_normal((30, 6, 3)), rng.random((30, 6))
    draws = lambda t: (zs[t], us[t])
    a = sref.run(ref.diag_gauss(sigma), x0, 0.4, 4, 10, 20, mode, draws)
    b = ref.run(ref.diag_gauss(sigma), x0, 0.4, 4, 10, 20, mode, draws)
    for k in ("samples", "eps", "eps_bar", "q", "accepted"):
        np.testing.assert_array_equal(a[k], b[k])
    assert a["margin"] == b["margin"]
    assert np.all((a["accept_stat"] >= 0) & (a["accept_stat"] <= 1))
    np.testing.assert_array_equal(a["divergent"] & a["accepted"], False)
    if mode == 0:
        assert not a["divergent"].any()
        np.testing.assert_array_equal(a["step_size"], np.full((30, 6), 0.4))
    else:
        assert np.all(a["step_size"][1:20] != 0.4)
        np.testing.assert_array_equal(a["step_size"][20:], np.broadcast_to(a["eps"], (10, 6)))
    # the energy is K0 - logp of the state the transition starts from
    lp0 = ref.diag_gauss(sigma)(x0)[0]
    np.testing.assert_allclose(a["energy"][0], 0.5 * np.sum(zs[0] ** 2, axis=1) - lp0, rtol=1e-15)


def test_new_symbols_are_declared_bound_and_exported():
    import general_mcmc_amd as g
    lib = g._lib.load()
    for n in NEW_SYMBOLS:
        assert n in g._lib.SIGNATURES
        assert hasattr(lib, n)


def test_facade_names():
    import general_mcmc_amd as g
    from general_mcmc_amd._sampler import DeviceSamples
    for name in ("collect_stats", "last_stats"):
        assert callable(getattr(g.HMC, name)) and callable(getattr(g.NUTS, name))
    assert isinstance(DeviceSamples.stats, property) and callable(DeviceSamples.logp)
    for name in ("energy", "accept_stat", "step_size", "n_leapfrog", "tree_depth", "divergent", "accepted"):
        assert isinstance(getattr(g.SamplerStats, name), property)
    assert "SamplerStats" in g.__all__ and "StatsSummary" in g.__all__


def test_null_arguments_are_refused_without_a_device():
    import general_mcmc_amd as g
    lib, E = g._lib.load(), g._lib
    buf = np.zeros(64)
    n = C.c_int64()
    assert lib.gm_sampler_set_stats(None, 1) == E.GM_EINVAL
    assert lib.gm_sampler_stats_info(None, C.byref(n), None, None, None) == E.GM_EINVAL
    assert lib.gm_sampler_stats_field(None, 0, E.ptr(buf)) == E.GM_EINVAL
    assert lib.gm_sampler_stats_reduce(None, 0, 1, E.ptr(buf), E.ptr(buf)) == E.GM_EINVAL
    assert lib.gm_stats_reduce_device(None, 0, 4, 0, 4, 0, E.ptr(buf), E.ptr(buf)) == E.GM_EINVAL
    assert b"records is NULL" in lib.gm_last_error()
