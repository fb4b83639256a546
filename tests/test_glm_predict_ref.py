"""The GLM posterior prediction without a GPU: the numpy reference
(tests/_glm_predict_ref.py) against scipy, its bounds against a float32
emulation of the evaluation, the WAIC arithmetic, and every refusal of the C
ABI (validation runs before the first device call)."""
import ctypes as C

import numpy as np
import pytest

from tests import _glm_predict_ref as P
from tests import _glm_ref as R


def _plan():
    import general_mcmc_amd as gm
    return gm.stats.predict_plan()


def test_plan_sizes():
    p = _plan()
    assert p["mfma_draws"] == 16 and p["tile_rows"] % 16 == 0 and p["slab_draws"] % 32 == 0
    import general_mcmc_amd as gm
    v = (C.c_int32 * 3)(-1, -1, -1)
    assert gm._lib.load().gm_glm_predict_plan(v, 2) == 0 and v[2] == -1 and v[0] == p["slab_draws"]
    assert gm._lib.load().gm_glm_predict_plan(None, 3) == gm._lib.GM_EINVAL


@pytest.mark.parametrize("family", R.FAMILIES)
def test_reference_against_scipy(family):
    from scipy.special import gammaln, logsumexp
    case = P.synth_case(17, 5, family, np.float64, 15)
    out = P.predict(case)
    eta = case.theta @ case.X.T + case.off
    if family == "poisson_log":
        ll = case.y * eta - np.exp(eta) - gammaln(case.y + 1.0)
    else:
        ll = case.y * eta - np.logaddexp(0.0, eta)
    np.testing.assert_allclose(out["pointwise"], ll, rtol=1e-13, atol=1e-14)
    np.testing.assert_allclose(out["lppd"], logsumexp(ll, axis=0) - np.log(15.0), rtol=1e-13)
    np.testing.assert_allclose(out["ll_var"], ll.var(axis=0, ddof=1), rtol=1e-10)
    np.testing.assert_allclose(out["eta_sd"], eta.std(axis=0, ddof=1), rtol=1e-13)
    np.testing.assert_allclose(P.lgamma1(case.y), gammaln(case.y + 1.0), rtol=1e-14, atol=1e-15)


def test_reference_non_finite_rules():
    ll = np.array([[-np.inf, -1.0, -2.0], [-np.inf, -np.inf, np.nan]])
    lp = P.lppd_of(ll)
    assert lp[0] == -np.inf and np.isnan(lp[2])
    assert abs(lp[1] - (-1.0 - np.log(2.0))) < 1e-15
    r = P.reduce(ll, ll, ll)
    assert r["ll_mean"][1] == -np.inf and np.isnan(r["ll_var"][0]) and np.isnan(r["ll_var"][1])
    one = P.reduce(ll[:1], ll[:1], ll[:1])
    assert np.all(np.isnan(one["eta_sd"])) and np.all(np.isnan(one["ll_var"]))


def _emulation_ratios(M, D, family, S):
    case = P.synth_case(M, D, family, np.float32, S)
    ref, bnd = P.predict(case), P.bounds(case)
    eta, mu, ll = P.emulate_f32(case)
    got = P.reduce(eta, mu, ll)
    got["pointwise"] = ll
    return P.ratios(got, ref, bnd, P.OUTPUTS + ("pointwise",))


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("shape", P.SHAPES)
def test_bounds_hold_for_a_float32_emulation(shape, family):
    """A sequential float32 sum with two roundings per term (worse than the
    device's fma chain) stays inside every bound at every GPU-test shape; at
    (17, 5) also at every draw count of the GPU tests."""
    M, D = shape
    counts = P.draw_counts(_plan()["slab_draws"]) if shape == (17, 5) else [15, 300]
    worst = {}
    for S in counts:
        for n, v in _emulation_ratios(M, D, family, S).items():
            worst[n] = max(worst.get(n, 0.0), v)
    print(f"{shape} {family}: worst fraction of the bound {worst}")
    assert max(worst.values()) <= 1.0
    # the bounds are not vacuous: a float32 evaluation uses a visible part of them
    if D >= 5:
        assert worst["pointwise"] > 1e-3


def test_waic_arithmetic_on_a_hand_made_matrix():
    import general_mcmc_amd as gm
    ll = np.log(np.array([[0.5, 0.25, 0.1], [0.4, 0.25, 0.4], [0.3, 0.25, 0.9], [0.5, 0.25, 0.05]]))
    r = P.reduce(ll, ll, ll)
    pred = gm.GLMPrediction(r["eta_mean"], r["eta_sd"], r["mu_mean"], r["mu_sd"], r["lppd"], r["ll_mean"],
                            r["ll_var"], None, 4)
    lppd = np.log(np.array([(0.5 + 0.4 + 0.3 + 0.5) / 4, 0.25, (0.1 + 0.4 + 0.9 + 0.05) / 4]))
    np.testing.assert_allclose(pred.lppd, lppd, rtol=1e-14)
    var = np.array([np.var(ll[:, j], ddof=1) for j in range(3)])
    assert var[1] == 0.0 and var[2] > 0.4 > var[0]
    w = pred.waic()
    elpd = lppd - var
    assert abs(w.elpd_waic - elpd.sum()) < 1e-14 and abs(w.p_waic - var.sum()) < 1e-14
    assert abs(w.waic + 2 * elpd.sum()) < 1e-13
    assert abs(w.se - np.sqrt(3 * np.var(elpd, ddof=1))) < 1e-14
    assert w.n_high_variance == 1
    np.testing.assert_allclose(w.pointwise, elpd, rtol=1e-14)
    assert abs(pred.lppd_total - lppd.sum()) < 1e-14
    ref = P.waic(r["lppd"], r["ll_var"])
    assert ref["elpd_waic"] == w.elpd_waic and ref["se"] == w.se and ref["n_high_variance"] == 1
    assert "elpd_waic" in str(w) and "lppd" in str(pred)
    no_y = gm.GLMPrediction(r["eta_mean"], r["eta_sd"], r["mu_mean"], r["mu_sd"], None, None, None, None, 4)
    with pytest.raises(ValueError, match="need y"):
        no_y.waic()
    assert "lppd" not in str(no_y)


def _call(lib, gm, *, family=1, dim=2, n_rows=3, x="ok", y="ok", offset=None, dtype=0, draws="ok", n_draws=4,
          stride=None, out="ok", want=("eta_mean",), device=False, model=True, pointwise=False):
    dp = C.POINTER(C.c_double)
    keep = []

    def arr(v, default):
        if v is None:
            return None
        a = np.ascontiguousarray(default if isinstance(v, str) else v, dtype=np.float64)
        keep.append(a)
        return a.ctypes.data_as(dp)

    rows = max(int(n_rows), 1) if n_rows < 100 else 3
    desc = gm._lib.gm_glm_desc()
    desc.family, desc.n_rows = family, n_rows
    desc.x = arr(x, np.ones((rows, max(dim, 1))))
    desc.y = arr(y, np.zeros(rows))
    desc.offset = arr(offset, None)
    desc.prior_sd = None
    o = gm._lib.gm_glm_predict_out()
    for n in want:
        a = np.empty(rows)
        keep.append(a)
        setattr(o, n, a.ctypes.data)
    if pointwise:
        o.pointwise = 1  # never written: the call is refused first
    th = np.zeros((4, max(dim, 1)), dtype=np.float32 if dtype == 0 else np.float64)
    d = gm._lib.ptr(th) if draws == "ok" else None
    mp = C.byref(desc) if model else None
    op = C.byref(o) if out == "ok" else None
    if device:
        rc = lib.gm_glm_predict_device(mp, dim, dtype, d, n_draws, dim if stride is None else stride, op)
    else:
        rc = lib.gm_glm_predict(mp, dim, dtype, d, n_draws, op)
    return rc, (lib.gm_last_error() or b"").decode()


def test_every_refusal_of_the_abi_and_its_message():
    """Each GM_EINVAL of gm_glm_predict / gm_glm_predict_device with its
    message; no device is touched (the draws pointer of the device variant is
    host memory that a kernel would fault on)."""
    import general_mcmc_amd as gm
    lib = gm._lib.load()
    nan, inf = np.nan, np.inf
    cases = [
        (dict(model=False), "the model (gm_glm_desc) is NULL"),
        (dict(family=3), "GLM target: family must be GM_GLM_BERNOULLI_LOGIT (1) or GM_GLM_POISSON_LOG (2)"),
        (dict(dim=0), "GLM target: dim must be in [1, 128]"),
        (dict(dim=129), "GLM target: dim must be in [1, 128]"),
        (dict(n_rows=0), "GLM target: n_rows must be >= 1"),
        (dict(n_rows=(1 << 24) + 1), "GLM target: n_rows must be <= 2^24"),
        (dict(x=None), "x must not be NULL"),
        (dict(dtype=2), "bad dtype"),
        (dict(draws=None), "draws is NULL"),
        (dict(n_draws=0), "n_draws must be >= 1"),
        (dict(device=True, stride=1), "stride_draw must be >= dim"),
        (dict(out=None), "out is NULL"),
        (dict(y=None, want=("lppd",)), "lppd, ll_mean, ll_var and pointwise need y"),
        (dict(y=None, want=("ll_mean",)), "need y"),
        (dict(y=None, want=("ll_var",)), "need y"),
        (dict(y=None, pointwise=True), "need y"),
        (dict(pointwise=True, n_draws=(1 << 31) // (4 * 3) + 1), "larger than 2^31 bytes: pass the rows in blocks"),
        (dict(pointwise=True, dtype=1, n_draws=(1 << 31) // (8 * 3) + 1), "pass the rows in blocks"),
        (dict(x=[[1, 1], [1, nan], [inf, 1]]), "GLM target: x is not finite at row 1, column 1"),
        (dict(y=[0, nan, 0]), "GLM target: y is not finite at row 1"),
        (dict(y=[0, 1, 1.5]), "GLM target: bernoulli_logit needs 0 <= y <= 1 at row 2"),
        (dict(family=2, y=[0, -1, 3]), "GLM target: poisson_log needs y >= 0 at row 1"),
        (dict(offset=[0, 0, -inf]), "GLM target: offset is not finite at row 2"),
        # the first offending row wins, whatever its kind; within a row x, y, its range, the offset
        (dict(x=[[1, 1], [1, 1], [nan, 1]], y=[0, inf, 0]), "GLM target: y is not finite at row 1"),
        (dict(x=[[1, 1], [1, nan], [1, 1]], y=[0, 2, 0], offset=[nan, 0, 0]),
         "GLM target: offset is not finite at row 0"),
    ]
    for device in (False, True):
        for kw, msg in cases:
            kw = dict(kw)
            if kw.pop("device", False) and not device:
                continue
            rc, err = _call(lib, gm, device=device, **kw)
            assert rc == gm._lib.GM_EINVAL, (kw, rc, err)
            assert msg in err, (kw, err)
    # without y the scan still covers x to the last row (a valid call would go on to the device)
    rc, err = _call(lib, gm, y=None, x=[[1, 1], [1, 1], [1, nan]])
    assert rc == gm._lib.GM_EINVAL and "x is not finite at row 2, column 1" in err


def test_new_symbols_are_declared_bound_and_exported():
    import general_mcmc_amd as gm
    from tests.test_abi import header_functions
    lib = gm._lib.load()
    for n in ("gm_glm_predict", "gm_glm_predict_device", "gm_glm_predict_plan"):
        assert n in header_functions() and n in gm._lib.SIGNATURES and hasattr(lib, n)
    assert C.sizeof(gm._lib.gm_glm_predict_out) == 8 * C.sizeof(C.c_void_p)


def test_facade_refusals_without_a_device():
    import general_mcmc_amd as gm
    X = np.ones((4, 2))
    t = gm.GLM(X, np.array([0.0, 1.0, 1.0, 0.0]))
    th = np.zeros((3, 2))
    with pytest.raises(ValueError, match="go with a new X"):
        t.predict(th, y=np.zeros(4))
    with pytest.raises(ValueError, match=r"X must be \[n_rows, dim\]"):
        t.predict(th, X=np.ones((4, 3)))
    with pytest.raises(ValueError, match="needs y"):
        t.predict(th, X=np.ones((5, 2)), pointwise=True)
    with pytest.raises(ValueError, match=r"draws must be \[\.\.\., dim\]"):
        t.predict(np.zeros((3, 5)))
    with pytest.raises(ValueError, match=r"y must be \[n_rows\]"):
        t.predict(th, X=np.ones((5, 2)), y=np.zeros(4))
    # the cap is checked before the matrix is allocated
    big = np.broadcast_to(np.zeros(2, dtype=np.float32), (1 << 28, 2))
    with pytest.raises(ValueError, match="2\\^31 bytes: pass the rows in blocks"):
        t.predict(big[: (1 << 27) + 1], pointwise=True)
