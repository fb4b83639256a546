"""GLM posterior prediction on the device (GLM.predict, gm_glm_predict*):
parity with the float64 reference inside the derived bounds of
tests/_glm_predict_ref.py, placement of every draw and row, the DeviceSamples
path, repeatability, non-finite values, new X and the refusals, WAIC."""
import ctypes as C

import numpy as np
import pytest

from tests import _glm_predict_ref as P
from tests import _glm_ref as R

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
ALL = P.OUTPUTS + ("pointwise",)


def _target(gm, case):
    """A gm.GLM on the case's (already rounded) data."""
    y = case.y if case.y is not None else np.zeros(case.M)
    return gm.GLM(case.X, y, family=case.family, offset=case.off)


def _got(pred):
    d = {n: getattr(pred, n) for n in P.OUTPUTS}
    d["pointwise"] = pred.pointwise
    return d


def _bits(a, b):
    """Bitwise equality of two predictions (NaNs by their place)."""
    for n in ALL:
        x, y = getattr(a, n), getattr(b, n)
        assert (x is None) == (y is None), n
        if x is not None:
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), f"{n} differs"


def _counts(gm):
    return P.draw_counts(gm.stats.predict_plan()["slab_draws"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("shape", P.SHAPES)
def test_parity_with_the_float64_reference(gm, shape, family, dtype):
    """Every output inside its derived bound at every draw count: 1, a partial
    matrix-core tile, 300, a second slab of one draw, two slabs and 15."""
    M, D = shape
    worst = {}
    for S in _counts(gm):
        case = P.synth_case(M, D, family, dtype, S)
        pred = _target(gm, case).predict(case.theta.astype(dtype), pointwise=True)
        assert pred.pointwise.dtype == dtype and pred.pointwise.shape == (S, M) and pred.n_draws == S
        q = P.ratios(_got(pred), P.predict(case), P.bounds(case), ALL)
        print(f"{shape} {family} {np.dtype(dtype).name} S={S}: fraction of the bound {q}")
        if S == 1:
            assert np.all(np.isnan(pred.eta_sd)) and np.all(np.isnan(pred.mu_sd)) and np.all(np.isnan(pred.ll_var))
        for n, v in q.items():
            worst[n] = max(worst.get(n, 0.0), v)
    print(f"{shape} {family} {np.dtype(dtype).name}: worst {worst}")
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_every_draw_lands_in_its_own_pointwise_row(gm, family, dtype):
    """Asymmetric data: pointwise row s of the whole call is the call on draw s
    alone, bit for bit (a swapped C/D map puts 3 of 4 draws in the wrong row)."""
    M, D, S = 70, 33, 40
    case = P.synth_case(M, D, family, dtype, S)
    t = _target(gm, case)
    th = case.theta.astype(dtype)
    whole = t.predict(th, pointwise=True)
    for s in range(S):
        one = t.predict(th[s], pointwise=True)
        assert one.pointwise.tobytes() == whole.pointwise[s].tobytes(), f"draw {s}"
        assert one.lppd.tobytes() == whole.pointwise[s].astype(np.float64).tobytes(), f"draw {s}: lppd of one draw"
    # the rows differ from each other and from their neighbours' (the data are not symmetric)
    assert len({whole.pointwise[s].tobytes() for s in range(S)}) == S


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_permuting_the_data_rows_permutes_every_output(gm, family, dtype):
    M, D, S = 70, 33, 300
    case = P.synth_case(M, D, family, dtype, S)
    th = case.theta.astype(dtype)
    a = _target(gm, case).predict(th, pointwise=True)
    perm = np.random.default_rng(2).permutation(M)
    b = gm.GLM(case.X[perm], case.y[perm], family=family, offset=case.off[perm]).predict(th, pointwise=True)
    for n in P.OUTPUTS:
        assert getattr(a, n)[perm].tobytes() == getattr(b, n).tobytes(), n
    assert np.ascontiguousarray(a.pointwise[:, perm]).tobytes() == b.pointwise.tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_repeatable_and_the_same_from_host_and_device_draws(gm, dtype):
    """Two calls give identical bits, and so do the host and the device entry
    point (with a draw stride larger than dim)."""
    from general_mcmc_amd.batch_vector import DeviceMatrix
    M, D = 70, 33
    S = gm.stats.predict_plan()["slab_draws"] + 17
    case = P.synth_case(M, D, "poisson_log", dtype, S)
    t = _target(gm, case)
    th = case.theta.astype(dtype)
    a = t.predict(th, pointwise=True)
    _bits(a, t.predict(th, pointwise=True))
    stride = D + 3
    wide = np.full((S, stride), np.nan, dtype=dtype)
    wide[:, :D] = th
    dev = DeviceMatrix(wide.shape, dtype)
    lib = gm._lib.load()
    try:
        gm._lib.check(lib.gm_memcpy_htod(C.c_void_p(dev.ptr), gm._lib.ptr(wide), wide.nbytes))
        dp = C.POINTER(C.c_double)
        desc = gm._lib.gm_glm_desc()
        desc.family, desc.n_rows = gm.GLM.FAMILIES["poisson_log"], M
        desc.x, desc.y, desc.offset = (v.ctypes.data_as(dp) for v in (t.X, t.y, t.offset))
        f = {n: np.empty(M) for n in P.OUTPUTS}
        pw = np.empty((S, M), dtype=dtype)
        out = gm._lib.gm_glm_predict_out(pointwise=pw.ctypes.data, **{n: v.ctypes.data for n, v in f.items()})
        gm._lib.check(lib.gm_glm_predict_device(C.byref(desc), D, gm._lib.dtype_code(dtype), C.c_void_p(dev.ptr), S,
                                                stride, C.byref(out)))
    finally:
        dev.close()
    for n in P.OUTPUTS:
        assert f[n].tobytes() == getattr(a, n).tobytes(), n
    assert pw.tobytes() == a.pointwise.tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_device_samples_of_a_run(gm, family, dtype):
    """The draws of a short HMC run, used where they lie: the bits of the same
    draws passed from the host in stored order; the joint log-density of every
    draw by the samplers' own evaluation (gm_target_logp_grad: DeviceSamples.logp
    goes through gm_bv_target_create, which refuses the GLM target) minus the
    prior term is the row sum of the pointwise ll without c, inside the two
    evaluation bounds added; a stale DeviceSamples raises."""
    M, D, chains = 70, 33, 6
    X, y, off = R.synth(M, D, family, 3)
    r = lambda v: np.asarray(v, dtype=dtype).astype(np.float64)
    X, y, off = r(X), r(y), r(off)
    target = gm.GLM(X, y, family=family, prior_sd=2.0, offset=off)
    x0 = (0.1 * np.random.default_rng(5).standard_normal((chains, D))).astype(dtype)
    s = gm.HMC(target, x0, 0.02, 5, dtype=dtype).set_seed(9)
    ds = s.run_positions(20, 10)
    host = np.ascontiguousarray(ds.to_host().transpose(1, 0, 2))  # stored order [n_collect, n_chains, dim]
    assert host.shape == (20, chains, D) and host.dtype == dtype
    a = target.predict(ds, pointwise=True)
    assert a.n_draws == 20 * chains
    _bits(a, target.predict(host, pointwise=True))
    # the joint log-density of every draw, by the sampler's own evaluation
    lp = target.unnorm_logp_batch(host.reshape(-1, D), dtype).astype(np.float64)  # stored order
    case = P.Case(X, y, off, family, host.reshape(-1, D), dtype)
    th = case.theta
    prior = 0.5 * np.sum(th * th / 4.0, axis=1)
    rows = np.sum(a.pointwise.astype(np.float64) - case.c, axis=1)
    ref = R.GlmRef(X, y, family, 2.0, off)
    S_scale, _ = ref.scales(th)
    u = R.unit_roundoff(dtype)
    bound = R.bound(ref, dtype) * S_scale + np.sum(P.bounds(case)["pointwise"] + u * np.abs(case.c), axis=1)
    q = np.abs((lp + prior) - rows) / bound
    print(f"{family} {np.dtype(dtype).name}: |logp + prior - sum ll| / bound = {float(np.max(q)):.3e}")
    assert float(np.max(q)) <= 1.0
    # moved draws: the comparison is of more than the start
    assert len({host[k].tobytes() for k in range(20)}) > 1
    s.run_positions(2, 0)
    with pytest.raises(RuntimeError, match="stale"):
        target.predict(ds)
    other = gm.GLM(X[:, :5], y, family=family, offset=off)
    with pytest.raises(ValueError, match="dim"):
        other.predict(s.run_positions(2, 0))
    s.close()


@pytest.mark.parametrize("dtype,big", [(np.float32, 100.0), (np.float64, 800.0)])
def test_bernoulli_far_in_both_tails_is_finite(gm, dtype, big):
    """|eta| = 100 (f32) and 800 (f64): every output finite and inside the bounds.

    The bounds are relative (the standard model without underflow). In float32
    exp(-100) = 3.7e-44 is subnormal, so it, log1p of it and the quotient mu
    carry an absolute error of up to half the smallest subnormal each, whatever
    the algorithm: the pointwise bound gets two smallest subnormals added here
    (measured without them: 177 times the relative bound of 3.6e-48 on the
    entry y = 0, eta = -100, ll = -3.7e-44, i.e. 6.4e-46 = 0.46 of one
    subnormal step). In float64 exp(-800) is 0 and the term adds nothing."""
    X = np.array([[big], [-big], [big], [-big], [0.5]])
    y = np.array([1.0, 1.0, 0.0, 0.0, 1.0])
    th = np.array([[1.0], [-1.0], [1.0], [0.5]])
    case = P.Case(X, y, None, "bernoulli_logit", th, dtype)
    assert np.max(np.abs(case.theta @ case.X.T)) == big
    pred = gm.GLM(X, y).predict(th.astype(dtype), pointwise=True)
    for n in ALL:
        assert np.all(np.isfinite(getattr(pred, n))), n
    bnd = P.bounds(case)
    bnd["pointwise"] = bnd["pointwise"] + 2.0 * float(np.finfo(dtype).smallest_subnormal)
    q = P.ratios(_got(pred), P.predict(case), bnd, ALL)
    print(f"{np.dtype(dtype).name}: fraction of the bound {q}")
    assert max(q.values()) <= 1.0


def test_poisson_overflow_on_one_row(gm):
    """Three draws, all with eta > 710 on row 0 only: every ll of that row is
    -inf, so its lppd is -inf (not NaN), its ll_var NaN; the other rows finite."""
    X = np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 0.5], [0.0, -1.0]])
    y = np.array([3.0, 1.0, 0.0, 2.0])
    th = np.array([[720.0, 0.1], [750.0, -0.3], [711.0, 0.4]])
    pred = gm.GLM(X, y, family="poisson_log").predict(th, pointwise=True)
    assert np.all(np.isneginf(pred.pointwise[:, 0])) and np.all(np.isfinite(pred.pointwise[:, 1:]))
    assert pred.lppd[0] == -np.inf and pred.ll_mean[0] == -np.inf and np.isnan(pred.ll_var[0])
    assert pred.mu_mean[0] == np.inf and np.isfinite(pred.eta_mean[0]) and np.isfinite(pred.eta_sd[0])
    for n in P.OUTPUTS:
        assert np.all(np.isfinite(getattr(pred, n)[1:])), n
    case = P.Case(X, y, None, "poisson_log", th, np.float64)
    q = P.ratios(_got(pred), P.predict(case), P.bounds(case), ALL)
    assert max(q.values()) <= 1.0
    # -inf in some draws only: nothing added to the lppd sum, ll_mean -inf
    th2 = np.array([[720.0, 0.1], [1.0, -0.3], [0.5, 0.4], [0.2, 0.0]])
    p2 = gm.GLM(X, y, family="poisson_log").predict(th2, pointwise=True)
    case2 = P.Case(X, y, None, "poisson_log", th2, np.float64)
    assert np.isfinite(p2.lppd[0]) and p2.ll_mean[0] == -np.inf and np.isnan(p2.ll_var[0])
    assert max(P.ratios(_got(p2), P.predict(case2), P.bounds(case2), ALL).values()) <= 1.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_nan_coefficient_in_one_draw_gives_nan_rows(gm, dtype):
    case = P.synth_case(17, 5, "bernoulli_logit", dtype, 40)
    th = case.theta.astype(dtype)
    th[23, 2] = np.nan
    pred = _target(gm, case).predict(th, pointwise=True)
    for n in P.OUTPUTS:
        assert np.all(np.isnan(getattr(pred, n))), n
    assert np.all(np.isnan(pred.pointwise[23])) and np.all(np.isfinite(np.delete(pred.pointwise, 23, axis=0)))


def test_new_rows_and_refusals(gm):
    case = P.synth_case(70, 33, "poisson_log", np.float32, 64)
    t = _target(gm, case)
    th = case.theta.astype(np.float32)
    Xn = np.random.default_rng(8).standard_normal((19, 33)).astype(np.float32).astype(np.float64) / 6.0
    pred = t.predict(th, X=Xn)
    assert pred.lppd is None and pred.ll_mean is None and pred.ll_var is None and pred.pointwise is None
    new = P.Case(Xn, None, None, "poisson_log", th, np.float32)
    names = ("eta_mean", "eta_sd", "mu_mean", "mu_sd")
    q = P.ratios({n: getattr(pred, n) for n in names}, P.predict(new), P.bounds(new), names)
    assert max(q.values()) <= 1.0
    with pytest.raises(ValueError, match="need y"):
        pred.waic()
    with pytest.raises(ValueError, match="needs y"):
        t.predict(th, X=Xn, pointwise=True)
    # with y and an offset for the new rows: the full set
    yn = np.arange(19.0) % 4
    on = np.linspace(-0.5, 0.5, 19).astype(np.float32).astype(np.float64)
    full = t.predict(th, X=Xn, y=yn, offset=on, pointwise=True)
    c2 = P.Case(Xn, yn, on, "poisson_log", th, np.float32)
    assert max(P.ratios(_got(full), P.predict(c2), P.bounds(c2), ALL).values()) <= 1.0
    # the 2^31-byte cap: refused before anything of that size exists
    big = np.broadcast_to(np.zeros(33, dtype=np.float32), ((1 << 31) // (4 * 70) + 1, 33))
    with pytest.raises(ValueError, match="pass the rows in blocks"):
        t.predict(big, pointwise=True)
    with pytest.raises(gm.GMError, match="x is not finite at row 1, column 0"):
        t.predict(th, X=np.array([[0.0] * 33, [np.inf] * 33]))


def test_waic_against_the_reference(gm):
    """(300, 5), 300 draws: waic() of the device's lppd and ll_var against the
    reference's, inside the bounds propagated through its sums."""
    for family in R.FAMILIES:
        for dtype in DTYPES:
            case = P.synth_case(300, 5, family, dtype, 300)
            pred = _target(gm, case).predict(case.theta.astype(dtype))
            ref, b = P.predict(case), P.bounds(case)
            w, rw = pred.waic(), P.waic(ref["lppd"], ref["ll_var"])
            be = b["lppd"] + b["ll_var"]  # per-row bound of elpd_i
            assert abs(w.elpd_waic - rw["elpd_waic"]) <= np.sum(be)
            assert abs(w.waic - rw["waic"]) <= 2 * np.sum(be)
            assert abs(w.p_waic - rw["p_waic"]) <= np.sum(b["ll_var"])
            assert np.all(np.abs(w.pointwise - rw["pointwise"]) <= be)
            # se = sqrt(M var): d var <= (2 sd_e |d e|_max + |d e|_max^2) M / (M - 1), through the root
            de = float(np.max(be))
            sd_e = float(np.std(rw["pointwise"], ddof=1))
            dvar = (2 * sd_e * de + de * de) * 300 / 299
            assert abs(w.se - rw["se"]) <= np.sqrt(300.0) * dvar / (2 * sd_e) * (1 + 1e-9) + 1e-15
            assert w.p_waic > 0
            assert abs(pred.lppd_total - float(np.sum(ref["lppd"]))) <= np.sum(b["lppd"])
