"""MH warm-up on the GPU: a per-chain proposal scale, a per-chain diagonal
proposal shape and their adaptation (gm_mh_set_adaptation /
gm_mh_set_proposal_scales / gm_mh_set_proposal_diag; mh_adapt_kernel).

1. equal scales + the all-ones shape give the CPU oracle's bits at every
   compiled layout (the MODE 0 kernel);
2. chain c with its own scale is the one-chain plain sampler of that scale;
3. a power-of-two shape is an exact reparametrisation of the target;
4. the adaptation recurrences follow the numpy float64 transcription
   (tests/_mh_adapt_ref.py) driven by the engine's own draws;
5. launch cuts, the run calls and the chain count do not change a bit;
6. a warmed-up or armed sampler resumes from a checkpoint bit for bit;
7. arming and the run calls;
8. user targets (runtime-compiled) take the same path;
9. on a badly scaled Gaussian the warm-up does what it is for;
10. the error paths.
"""
import ctypes as C

import numpy as np
import pytest

from tests import _layout_cases as lc
from tests import _mh_adapt_ref as ref
from tests import custom_targets as ct

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
dtypes = pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
TAG_MH_PROP, TAG_MH_ACC = 4, 5


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


def _mh(gm, target, std, x0, dtype, **kw):
    return gm.MetropolisHastings(target, gm.IsotropicGaussian(std), x0, dtype=dtype, **kw)


def _state(s):
    return s.proposal_scales() + (s.proposal_diag(), s.positions(), s.accept_counts())


def _same_state(a, b):
    for x, y in zip(_state(a), _state(b)):
        np.testing.assert_array_equal(x, y)


# ---- 1. the layout matrix: MODE 0 against the CPU oracle ----------------------
@dtypes
@pytest.mark.parametrize("lay,dim", lc.CASES, ids=lc.CASE_IDS)
def test_equal_scales_are_the_oracle_at_every_layout(gm, oracle, lay, dim, dtype):
    x0 = lc.start(gm, dim, dtype)
    std = lc.mh_prop_std(dim)
    for name in lc.TARGETS:
        s = _mh(gm, lc.target(gm, name, dim), std, x0, dtype, chain_offset=lc.CHAIN_OFFSET).seed(lc.MH_SEED)
        s.set_layout(*lay)
        s.set_proposal_scales(np.full(lc.N_CHAINS, std))
        assert s.layout() == lay
        step0 = 0
        for (nc, nd), (samples, acc) in zip(lc.MH_RUNS, lc.mh_reference(gm, oracle, name, lay, dim, dtype)):
            msg = f"{name}: run({nc}, {nd}) from step {step0}"
            np.testing.assert_array_equal(s.run(nc, nd), samples, err_msg=msg)
            np.testing.assert_array_equal(s.accept_counts(), acc, err_msg=msg)
            step0 += nc + nd
        if (name, dim) not in lc.FLAT:  # both branches of the accept were taken
            assert 0 < s.accept_counts().sum() < lc.MH_TRANSITIONS * lc.N_CHAINS, name
        s.close()


# ---- 2. per-chain scales -----------------------------------------------------
@dtypes
@pytest.mark.parametrize("dim", [3, 65])
def test_per_chain_scale_is_that_chains_plain_sampler(gm, dtype, dim):
    n_chains, std = 9, 0.3 / np.sqrt(dim)
    x0 = (gm.init_with_seed(n_chains, dim, 12, np.float64) * 0.5).astype(dtype)
    scales = std * (1.0 + np.arange(n_chains) / 8.0)
    s = _mh(gm, gm.RosenbrockND(), std, x0, dtype).seed(8).set_proposal_scales(scales)
    out = s.run(70, 3)
    np.testing.assert_array_equal(s.proposal_scales()[0], scales.astype(dtype).astype(np.float64))
    for c in range(n_chains):
        one = _mh(gm, gm.RosenbrockND(), float(dtype(scales[c])), x0[c:c + 1], dtype, chain_offset=c).seed(8)
        np.testing.assert_array_equal(one.run(70, 3)[0], out[c])
        np.testing.assert_array_equal(one.positions()[0], s.positions()[c])
        assert one.accept_counts()[0] == s.accept_counts()[c]
        one.close()
    assert 0 < s.accept_counts().sum() < 73 * n_chains


# ---- 3. the shape as an exact reparametrisation -------------------------------
@dtypes
def test_power_of_two_shape_is_an_exact_reparametrisation(gm, dtype):
    """Sampler A: target (mu, P) with shape s. Sampler B, plain: target
    (mu/s, diag(s) P diag(s)) from x/s. Every difference between the two is a
    scaling by a power of two, so A's samples are s * B's bit for bit."""
    n_chains, dim = 33, 5
    s_ = np.array([1.0, 2.0, 0.25, 8.0, 0.5])
    mu = np.array([0.5, -1.0, 0.25, 2.0, -0.75])
    prec = 2.0 * np.eye(dim) - 0.5 * (np.eye(dim, k=1) + np.eye(dim, k=-1)) + 0.25 * (
        np.eye(dim, k=2) + np.eye(dim, k=-2))
    x = gm.init_with_seed(n_chains, dim, 13, np.float64).astype(dtype)
    a = _mh(gm, _prec_gauss(gm, mu, prec), 0.5, x, dtype).seed(4).set_proposal_diag(s_)
    b = _mh(gm, _prec_gauss(gm, mu / s_, prec * np.outer(s_, s_)), 0.5, (x / s_.astype(dtype)).astype(dtype),
            dtype).seed(4)
    np.testing.assert_array_equal(a.proposal_diag(), np.broadcast_to(s_.astype(dtype), (n_chains, dim)))
    np.testing.assert_array_equal(a.proposal_scales()[0], np.full(n_chains, 0.5))
    np.testing.assert_array_equal(a.run(70, 4), b.run(70, 4) * s_)
    np.testing.assert_array_equal(a.accept_counts(), b.accept_counts())
    assert 0 < a.accept_counts().sum() < 74 * n_chains  # both branches of the accept were taken


# ---- 4. the recurrences against the numpy transcription -----------------------
# name: (mode, n_collect, n_discard)
CASES = {"scale": (1, 20, 60), "diagonal": (2, 20, 60), "first_window": (2, 0, 26)}
_SIGMA4 = np.array([0.5, 1.0, 3.0])
_CFG4 = (0.234, 5, 10, 10, 0.05, 1e-6)
_BOUND4 = 1e-10  # not a measurement: see test_recurrences_follow_the_transcription


def _oracle_draws(oracle, n_chains, dim, seed, n):
    lib = oracle.lib
    zs = np.array([[[lib.or_tab_normal_d(seed, c, t, TAG_MH_PROP, i) for i in range(dim)] for c in range(n_chains)]
                   for t in range(n)])
    us = np.array([[lib.or_uniform_co_d(seed, c, t, TAG_MH_ACC, 0) for c in range(n_chains)] for t in range(n)])
    return lambda t: (zs[t], us[t])


@pytest.fixture(scope="module")
def recurrences(gm, oracle):
    """(GPU results, transcription) per case, the transcription driven by the
    engine's own proposal normals and accept uniforms (the oracle library's),
    at the first seed whose decisions are all clear of their thresholds."""
    n_chains, dim, std0 = 6, 3, 1.0
    x0 = gm.init_with_seed(n_chains, dim, 14, np.float64)
    logp = ref.diag_gauss_logp(_SIGMA4)
    for seed in range(1, 200):  # chosen on the CPU, from the transcription alone
        draws = _oracle_draws(oracle, n_chains, dim, seed, 80)
        rs = {case: ref.run(logp, x0, std0, nc, nd, mode, draws, *_CFG4) for case, (mode, nc, nd) in CASES.items()}
        if min(r["margin"] for r in rs.values()) >= 1e-9:
            break
    res = {}
    for case, (mode, n_collect, n_discard) in CASES.items():
        s = _mh(gm, _prec_gauss(gm, np.zeros(dim), np.diag(1.0 / _SIGMA4 ** 2)), std0, x0, np.float64)
        s.seed(seed).set_adaptation(gm.MHAdaptConfig(("none", "scale", "diagonal")[mode], *_CFG4))
        out = s.run(n_collect, n_discard)
        sc, bar = s.proposal_scales()
        gpu = dict(scale=sc, scale_bar=bar, diag=s.proposal_diag(), q=s.positions(), samples=out,
                   acc=s.accept_counts())
        res[case] = (gpu, rs[case])
        s.close()
    return res


@pytest.mark.parametrize("case", list(CASES))
def test_recurrences_follow_the_transcription(recurrences, case):
    """Within 1e-10 (scales and shape relative; positions and samples relative
    to the coordinate's sigma). The bound is reasoned, not measured: with equal
    decisions the position error is the accumulated rounding of <= 80 sums,
    the scale error the rounding of h_bar times the recurrence's gain
    sqrt(k)/gamma <= 155 through exp / log of a few ulp, together 1e-13 to
    1e-12; the 100x margin covers the device's gexp / glog; a semantic slip
    (wrong k, update before accept, wrong window) is >= 1e-4.
    Measured on an MI355X: see DESIGN.md, "MH warm-up"."""
    mode, n_collect, n_discard = CASES[case]
    # ends at 15, 25 and 45 are odd: the f64 Philox pair is cut there; the window ending at 49 has 4 positions
    assert ref.window_ends(60, 5, 10, 10) == [15, 25, 45, 49]
    assert ref.window_ends(26, 5, 10, 10) == [15]
    gpu, r = recurrences[case]
    assert r["margin"] >= 1e-9, r["margin"]
    dev = {k: float(np.max(np.abs(gpu[k] - r[k]) / np.abs(r[k]))) for k in ("scale", "scale_bar", "diag")}
    dev["q"] = float(np.max(np.abs(gpu["q"] - r["q"]) / _SIGMA4))
    if n_collect:
        dev["samples"] = float(np.max(np.abs(gpu["samples"] - r["samples"]) / _SIGMA4))
    print(f"{case}: deviation from the transcription {dev}, decision margin {r['margin']:.3e}")
    np.testing.assert_array_equal(gpu["acc"], r["accepted"].sum(axis=0))
    if n_collect:
        moved = np.any(gpu["samples"][:, 1:] != gpu["samples"][:, :-1], axis=2)
        np.testing.assert_array_equal(moved, r["accepted"][n_discard + 1:].T)
    if mode == 1:
        np.testing.assert_array_equal(gpu["diag"], np.ones_like(gpu["diag"]))
    else:
        assert np.all(gpu["diag"] != 1.0)
    if n_discard == 60:
        np.testing.assert_array_equal(gpu["scale"], gpu["scale_bar"])
    assert max(dev.values()) <= _BOUND4, dev


# ---- 5. launch cuts and chain independence ------------------------------------
@dtypes
@pytest.mark.parametrize("dim,std", [(64, 0.9), (7, 2.5)])
def test_launch_cuts_run_calls_and_chain_count_change_nothing(gm, dtype, dim, std):
    """64-D: the 64x1 layout crosses the accept window at step 64 in the middle
    of the warm-up (windows end at 15, 25, 45, 85, 139 of 150)."""
    n_chains = 70
    x0 = gm.init_with_seed(n_chains, dim, 18, np.float64).astype(dtype)
    cfg = gm.MHAdaptConfig("diagonal", 0.234, 5, 10, 10, 0.05, 1e-6)
    target = gm.IsotropicGaussian(3.0)

    def make(x=x0, **kw):
        return _mh(gm, target, std, x, dtype, **kw).seed(5).set_adaptation(cfg)

    a, b, c, d = make(), make(), make(), make()
    if dim == 64:
        assert a.layout() == (64, 1)
    out = a.run(10, 150)
    np.testing.assert_array_equal(b.set_steps_per_launch(7).run(10, 150), out)
    seen = []
    out_c, stats = c.run_progress(10, 150, progress=seen.append, interval=0.0)
    np.testing.assert_array_equal(out_c, out)
    assert stats is not None and seen and seen[-1].done == 160
    d.set_async(True)
    dev = d.run_positions(10, 150)
    d.synchronize()
    np.testing.assert_array_equal(dev.to_host().astype(np.float64), out)
    for s in (b, c, d):
        _same_state(a, s)
    sc, bar = a.proposal_scales()
    diag, q, acc = a.proposal_diag(), a.positions(), a.accept_counts()
    assert np.all(sc != std) and np.all(diag != 1.0) and 0 < acc.sum() < 160 * n_chains
    for ch in range(n_chains):
        one = make(x0[ch:ch + 1], chain_offset=ch)
        np.testing.assert_array_equal(one.run(10, 150)[0], out[ch])
        for x, y in zip(_state(one), (sc[ch:ch + 1], bar[ch:ch + 1], diag[ch:ch + 1], q[ch:ch + 1],
                                      acc[ch:ch + 1])):
            np.testing.assert_array_equal(x, y)
        one.close()


# ---- 6. checkpoint -----------------------------------------------------------
@dtypes
def test_warmed_up_and_armed_samplers_resume_bit_for_bit(gm, dtype):
    n_chains, dim = 40, 5
    x0 = gm.init_with_seed(n_chains, dim, 15, np.float64).astype(dtype)
    target = _prec_gauss(gm, np.zeros(dim), np.diag(1.0 / np.array([0.5, 1.0, 2.0, 4.0, 8.0]) ** 2))
    cfg = gm.MHAdaptConfig("diagonal", 0.234, 5, 10, 10, 0.05, 1e-6)
    a = _mh(gm, target, 1.0, x0, dtype).seed(6)
    plain_blob = a.save_state()
    a.set_adaptation(cfg)
    # armed, not yet run: the loaded sampler runs the warm-up
    b = _mh(gm, target, 1.0, x0, dtype).load_state(a.save_state())
    np.testing.assert_array_equal(a.run(5, 60), b.run(5, 60))
    _same_state(a, b)
    assert np.all(a.proposal_diag() != 1.0) and np.all(a.proposal_scales()[0] != 1.0)
    # warmed up: the loaded sampler continues
    blob = a.save_state()
    assert len(blob) > len(plain_blob)
    c = _mh(gm, target, 1.0, x0, dtype).load_state(blob)
    _same_state(a, c)
    np.testing.assert_array_equal(a.run(70, 0), c.run(70, 0))
    _same_state(a, c)
    assert c.save_state() == a.save_state()
    # scales alone carry no [chains, dim] arrays
    e = _mh(gm, target, 1.0, x0, dtype).seed(6).set_proposal_scales(np.full(n_chains, 0.7))
    assert len(plain_blob) < len(e.save_state()) < len(blob)
    # mode 0 drops the per-chain state: the blob is a plain sampler's again, and
    # a plain blob loaded into an adaptive sampler returns it to the plain path
    a.set_adaptation(gm.MHAdaptConfig("none"))
    assert len(a.save_state()) == len(plain_blob)
    c.load_state(plain_blob)
    assert c.save_state() == plain_blob
    np.testing.assert_array_equal(c.proposal_scales()[0], np.full(n_chains, 1.0))
    np.testing.assert_array_equal(c.proposal_diag(), np.ones((n_chains, dim), dtype=dtype))


# ---- 7. arming and the run calls ----------------------------------------------
def test_arming_and_the_run_calls(gm):
    n_chains, dim = 20, 4
    x0 = gm.init_with_seed(n_chains, dim, 17, np.float64)
    cfg = gm.MHAdaptConfig("scale")
    target = gm.IsotropicGaussian(1.5)
    s = _mh(gm, target, 0.2, x0, np.float64).seed(1)
    np.testing.assert_array_equal(s.proposal_scales()[0], np.full(n_chains, 0.2))
    np.testing.assert_array_equal(s.proposal_diag(), np.ones((n_chains, dim)))
    s.set_adaptation(cfg)
    s.run(3, 0)  # n_discard == 0: adapts nothing, stays armed
    s.step()     # a step never starts a warm-up
    np.testing.assert_array_equal(s.proposal_scales()[0], np.full(n_chains, 0.2))
    s.run(2, 30)
    sc, bar = s.proposal_scales()
    assert np.all(sc != 0.2) and np.all(sc > 0) and np.array_equal(sc, bar)  # frozen at scale_bar
    s.run(4, 10)  # not armed any more: the discarded transitions are plain burn-in
    s.step()
    np.testing.assert_array_equal(s.proposal_scales()[0], sc)
    np.testing.assert_array_equal(s.proposal_diag(), np.ones((n_chains, dim)))
    s.set_adaptation(cfg)  # re-armed: starts from the current scales
    s.run(0, 25)
    assert np.all(s.proposal_scales()[0] != sc)
    # mode 0: back on the creation proposal and the plain kernel
    s.set_adaptation(gm.MHAdaptConfig("none"))
    np.testing.assert_array_equal(s.proposal_scales()[0], np.full(n_chains, 0.2))
    p = _mh(gm, target, 0.2, s.positions(), np.float64).seed(9)
    s.seed(9)
    np.testing.assert_array_equal(s.run(5, 2), p.run(5, 2))


# ---- 8. user targets ---------------------------------------------------------
@dtypes
def test_custom_target(gm, dtype):
    dim, n_chains, std = 3, 70, 0.05
    x0 = (gm.init_with_seed(n_chains, dim, 19, np.float64) * 0.5).astype(dtype)
    t = gm.CustomTarget(ct.ROSENBROCK, dim, [1.0, 100.0])
    t.check("mh_adapt", dtype)
    pair = []
    for adaptive in (False, True):
        s = _mh(gm, t, std, x0, dtype, chain_offset=5).seed(3).set_steps_per_launch(30)
        if adaptive:
            s.set_proposal_scales(np.full(n_chains, std))
        pair.append(s)
    np.testing.assert_array_equal(pair[0].run(70, 5), pair[1].run(70, 5))
    np.testing.assert_array_equal(pair[0].positions(), pair[1].positions())
    np.testing.assert_array_equal(pair[0].accept_counts(), pair[1].accept_counts())
    assert 0 < pair[0].accept_counts().sum() < 75 * n_chains
    s = pair[1].set_adaptation(gm.MHAdaptConfig("diagonal", 0.234, 5, 10, 10, 0.05, 1e-6))
    out = s.run(5, 60)
    sc, bar = s.proposal_scales()
    diag = s.proposal_diag()
    assert np.all(np.isfinite(out))
    assert np.all(np.isfinite(sc)) and np.all(sc > 0) and np.all(sc != float(dtype(std)))
    assert np.all(np.isfinite(diag)) and np.all(diag > 0) and np.all(diag != 1.0)


# ---- 9. statistical ----------------------------------------------------------
@dtypes
def test_warmup_on_a_badly_scaled_gaussian(gm, dtype):
    """The shape and intervals of tests/test_mh_adapt_ref.py
    (tests/_mh_adapt_ref.py check_*), on the GPU."""
    dim = 8
    x0 = gm.init_with_seed(ref.N_CHAINS, dim, 20, np.float64).astype(dtype)
    target = _prec_gauss(gm, np.zeros(dim), np.diag(1.0 / ref.SIGMA ** 2))
    s = _mh(gm, target, 8.0, x0, dtype).seed(31)
    acc = ref.moves(s.run(ref.N_COLLECT, ref.N_DISCARD))
    print(f"control acceptance {acc:.4f}")
    ref.check_control(acc)
    for start in (8.0, 0.01):
        for name, check in (("scale", ref.check_mode1), ("diagonal", ref.check_mode2)):
            s = gm.MetropolisHastings.with_adaptation(target, gm.IsotropicGaussian(start), x0,
                                                      gm.MHAdaptConfig(name), dtype=dtype).seed(31)
            out = s.run(ref.N_COLLECT, ref.N_DISCARD)
            sc, bar = s.proposal_scales()
            diag = s.proposal_diag().astype(np.float64)
            print(f"start {start} {name}: acceptance {ref.moves(out):.3f}, median scale {np.median(sc):.3f}, "
                  f"median diag/sigma {np.median(diag / ref.SIGMA, axis=0)}, "
                  f"variance/sigma^2 {out.reshape(-1, dim).var(axis=0) / ref.SIGMA ** 2}, "
                  f"lag-1 {ref.lag1_autocorr(out, 7):.4f}")
            check(ref.moves(out), sc, bar, diag, out)
            s.close()


# ---- 10. error paths ---------------------------------------------------------
def _new_calls(gm, s):
    """Return codes of the five new entry points with valid arguments."""
    lib = gm._lib.load()
    n, d = s.n_chains, s.dim
    sc = np.full(n, 0.1)
    m = np.ones((n, d), dtype=s.dtype)
    out1, out2 = np.empty(n), np.empty(n)
    return [lib.gm_mh_set_adaptation(s._h, 1, 0.234, 75, 150, 25, 0.05, 1e-6),
            lib.gm_mh_set_proposal_scales(s._h, gm._lib.ptr(sc)),
            lib.gm_mh_get_proposal_scales(s._h, gm._lib.ptr(out1), gm._lib.ptr(out2)),
            lib.gm_mh_set_proposal_diag(s._h, gm._lib.ptr(m)),
            lib.gm_mh_get_proposal_diag(s._h, gm._lib.ptr(m))]


def test_error_paths(gm):
    L = gm._lib
    lib = L.load()
    x0 = gm.init_det(4, 3)
    hmc = gm.HMC(gm.IsotropicGaussian(1.0), x0, 0.1, 3)
    nuts = gm.NUTS(gm.IsotropicGaussian(1.0), x0, 0.8)
    assert _new_calls(gm, hmc) == [L.GM_ESTATE] * 5
    assert _new_calls(gm, nuts) == [L.GM_ESTATE] * 5

    for dtype in DTYPES:
        s = _mh(gm, gm.IsotropicGaussian(1.0), 0.5, x0.astype(dtype), dtype).seed(1)
        blob = s.save_state()
        for bad in (0.0, 1.0, float("nan"), -0.2, 1.5):
            assert lib.gm_mh_set_adaptation(s._h, 1, bad, 75, 150, 25, 0.05, 1e-6) == L.GM_EINVAL
        assert lib.gm_mh_set_adaptation(s._h, 3, 0.234, 75, 150, 25, 0.05, 1e-6) == L.GM_EINVAL
        assert lib.gm_mh_set_adaptation(s._h, 2, 0.234, -1, 150, 25, 0.05, 1e-6) == L.GM_EINVAL
        assert lib.gm_mh_set_adaptation(s._h, 2, 0.234, 75, 150, 25, 1.5, 1e-6) == L.GM_EINVAL
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            m = np.ones((4, 3), dtype=dtype)
            m[2, 1] = bad
            assert lib.gm_mh_set_proposal_diag(s._h, L.ptr(m)) == L.GM_EINVAL
            e = np.full(4, 0.1)
            e[3] = bad
            assert lib.gm_mh_set_proposal_scales(s._h, L.ptr(e)) == L.GM_EINVAL
        if dtype == np.float32:  # 2 scale^2 is not a normal float
            e = np.full(4, 0.1)
            e[0] = 1e-25
            assert lib.gm_mh_set_proposal_scales(s._h, L.ptr(e)) == L.GM_EINVAL
            tiny = _mh(gm, gm.IsotropicGaussian(1.0), 1e-25, x0.astype(dtype), dtype)
            tiny_blob = tiny.save_state()
            assert lib.gm_mh_set_adaptation(tiny._h, 2, 0.234, 75, 150, 25, 0.05, 1e-6) == L.GM_EINVAL
            assert lib.gm_mh_set_proposal_diag(tiny._h, L.ptr(np.ones((4, 3), dtype=dtype))) == L.GM_EINVAL
            assert tiny.save_state() == tiny_blob
        # nothing changed: still the plain sampler, byte for byte
        assert s.save_state() == blob
        np.testing.assert_array_equal(s.proposal_diag(), np.ones((4, 3), dtype=dtype))
        # a rejected shape leaves a set one in place
        good = np.full((4, 3), 4.0, dtype=dtype)
        s.set_proposal_diag(good)
        m = good.copy()
        m[0, 0] = -1.0
        assert lib.gm_mh_set_proposal_diag(s._h, L.ptr(m)) == L.GM_EINVAL
        np.testing.assert_array_equal(s.proposal_diag(), good)
        np.testing.assert_array_equal(s.proposal_scales()[0], np.full(4, 0.5))
