"""HMC, MH and NUTS (identity metric) against the CPU oracle, bit for bit, at
every compiled layout (GM_LAYOUT_LIST) x {D_full, D_pad} x {f32, f64} x the
three built-in targets: every instantiation of hmc_kernel, mh_kernel and
nuts_kernel is launched through its sampler by at least one
assert_array_equal, and hmc_adapt_kernel is tied to hmc_kernel at every
layout. The cases, their step sizes and the oracle's runs are in
tests/_layout_cases.py; tests/test_layout_matrix_cases.py checks on the CPU
that the list is the compiled one and that every case accepts and rejects.

Every run has 5 chains at global chain ids 3..7 (two workgroups at 64 lanes
per chain, a partly filled wave at narrower groups) and spans several
launches, so the state hand-off, the padded sample store and the draw-block
and accept-window positions of a launch that starts mid-block are part of
every case."""
import numpy as np
import pytest

from tests import _layout_cases as lc

pytestmark = pytest.mark.gpu

matrix = pytest.mark.parametrize("lay,dim", lc.CASES, ids=lc.CASE_IDS)
dtypes = pytest.mark.parametrize("dtype", lc.DTYPES, ids=["f32", "f64"])


@dtypes
@matrix
def test_hmc_layout_bitwise(gm, oracle, lay, dim, dtype):
    x0 = lc.start(gm, dim, dtype)
    for name in lc.TARGETS:
        s = gm.HMC(lc.target(gm, name, dim), x0, lc.HMC_EPS[name, dim], lc.HMC_L, dtype=dtype,
                   chain_offset=lc.CHAIN_OFFSET).set_seed(lc.HMC_SEED)
        s.set_layout(*lay)
        assert s.layout() == lay
        step0 = 0
        for (nc, nd), (samples, q, acc) in zip(lc.HMC_RUNS, lc.hmc_reference(gm, oracle, name, lay, dim, dtype)):
            msg = f"{name}: run({nc}, {nd}) from step {step0}"
            np.testing.assert_array_equal(s.run(nc, nd), samples, err_msg=msg)
            np.testing.assert_array_equal(s.positions(), q, err_msg=msg)
            np.testing.assert_array_equal(s.accept_counts(), acc, err_msg=msg)
            step0 += nc + nd
        s.close()


@dtypes
@matrix
def test_mh_layout_bitwise(gm, oracle, lay, dim, dtype):
    x0 = lc.start(gm, dim, dtype)
    prop = gm.IsotropicGaussian(lc.mh_prop_std(dim))
    for name in lc.TARGETS:
        s = gm.MetropolisHastings(lc.target(gm, name, dim), prop, x0, dtype=dtype,
                                  chain_offset=lc.CHAIN_OFFSET).seed(lc.MH_SEED)
        s.set_layout(*lay)
        assert s.layout() == lay
        step0 = 0
        for (nc, nd), (samples, acc) in zip(lc.MH_RUNS, lc.mh_reference(gm, oracle, name, lay, dim, dtype)):
            msg = f"{name}: run({nc}, {nd}) from step {step0}"
            np.testing.assert_array_equal(s.run(nc, nd), samples, err_msg=msg)
            np.testing.assert_array_equal(s.accept_counts(), acc, err_msg=msg)
            step0 += nc + nd
        s.close()


@dtypes
@matrix
def test_nuts_layout_bitwise(gm, oracle, lay, dim, dtype):
    x0 = lc.start(gm, dim, dtype)
    for name in lc.TARGETS:
        s = gm.NUTS(lc.target(gm, name, dim), x0, lc.NUTS_TARGET_ACCEPT, dtype=dtype, max_depth=lc.NUTS_MAX_DEPTH,
                    chain_offset=lc.CHAIN_OFFSET).set_seed(lc.NUTS_SEED)
        s.set_layout(*lay)
        assert s.layout() == lay
        s.set_steps_per_launch(lc.NUTS_STEPS_PER_LAUNCH)
        for (nc, nd), (samples, acc, nlf, eps, bar) in zip(lc.NUTS_RUNS,
                                                          lc.nuts_reference(gm, oracle, name, lay, dim, dtype)):
            msg = f"{name}: run({nc}, {nd})"
            np.testing.assert_array_equal(s.run(nc, nd), samples, err_msg=msg)
            np.testing.assert_array_equal(s.accept_counts(), acc, err_msg=msg)
            np.testing.assert_array_equal(s.leapfrog_counts(), nlf, err_msg=msg)
            got_eps, got_bar = s.step_sizes()
            np.testing.assert_array_equal(got_eps.astype(dtype), eps, err_msg=msg)
            np.testing.assert_array_equal(got_bar.astype(dtype), bar, err_msg=msg)
        s.close()


@dtypes
@pytest.mark.parametrize("lay", lc.LAYOUTS, ids=[f"{a}x{b}" for a, b in lc.LAYOUTS])
def test_hmc_adapt_equals_plain_at_every_layout(gm, lay, dtype):
    """hmc_adapt_kernel with equal per-chain step sizes and the identity
    metric gives hmc_kernel's bits at the same layout; with
    test_hmc_layout_bitwise that ties it to the oracle."""
    dim, n_chains = lc.dims(lay)[-1], 7
    x0 = lc.start(gm, dim, dtype, n_chains)
    for name in ("rosenbrock", "gauss"):
        eps = lc.HMC_EPS[name, dim]
        pair = []
        for adaptive in (False, True):
            s = gm.HMC(lc.target(gm, name, dim), x0, eps, lc.HMC_L, dtype=dtype,
                       chain_offset=lc.CHAIN_OFFSET).set_seed(lc.HMC_SEED)
            s.set_layout(*lay)
            s.set_steps_per_launch(3)
            if adaptive:
                s.set_step_sizes(np.full(n_chains, eps))
            assert s.layout() == lay
            pair.append(s)
        plain, adapt = pair
        np.testing.assert_array_equal(adapt.run(7, 5), plain.run(7, 5), err_msg=name)
        np.testing.assert_array_equal(adapt.positions(), plain.positions(), err_msg=name)
        np.testing.assert_array_equal(adapt.accept_counts(), plain.accept_counts(), err_msg=name)
        assert 0 < plain.accept_counts().sum() or (name, dim) in lc.FLAT
        for s in pair:
            s.close()
