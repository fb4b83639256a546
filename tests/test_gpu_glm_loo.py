"""GLM PSIS-LOO on the device (GLM.loo, gm_glm_loo*): the sorted raw tail bit
for bit against the pointwise matrix of GLM.predict, pareto_k and elpd_loo
against the float64 transcription of tests/_glm_loo_ref.py inside its fuzz
yardstick, large tails, row groups, repeatability and the entry points, draw
order, non-finite rows, small draw counts, an influential row, the refusals."""
import numpy as np
import pytest

from tests import _glm_loo_ref as L
from tests import _glm_predict_ref as P
from tests import _glm_ref as R

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
SHAPES = [(1, 1), (17, 5), (70, 33), (70, 128), (300, 64)]
FIELDS = ("elpd_loo", "pareto_k", "lppd", "tail")


def _target(gm, case):
    return gm.GLM(case.X, case.y, family=case.family, offset=case.off)


def _counts(gm):
    slab = gm.stats.predict_plan()["slab_draws"]
    return [25, 300, slab + 1, 2 * slab + 15]


def _bits(a, b, perm=None):
    """Bitwise equality of two GLMLoo (NaNs by their place); perm: a's rows in b's order."""
    for n in FIELDS:
        x, y = getattr(a, n), getattr(b, n)
        assert (x is None) == (y is None), n
        if x is not None:
            x = x if perm is None else np.ascontiguousarray(x[perm])
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), f"{n} differs"
    assert (a.tail_len, a.n_nonfinite, a.n_draws) == (b.tail_len, b.n_nonfinite, b.n_draws)


def _device_and_reference(gm, target, th, reff=1.0, **kw):
    """One loo call with its tail, the pointwise matrix of predict on the same
    draws, the transcription on that matrix and its sensitivity."""
    pw = target.predict(th, pointwise=True).pointwise
    got = target.loo(th, reff=reff, tail=True, **kw)
    ref = L.loo(pw, reff)
    return got, pw, ref, L.sensitivity(pw, reff, plain=ref)


def _assert_tail(got, pw, reff=1.0):
    want = L.raw_tail(pw, reff)
    assert got.tail.dtype == np.float64 and got.tail.shape == want.shape
    assert got.tail.tobytes() == want.tobytes(), "the sorted raw tail differs from predict's pointwise matrix"


def _assert_parity(got, ref, sens, label):
    dev = {"elpd_loo": got.elpd_loo, "pareto_k": got.pareto_k}
    q = L.ratios(dev, ref, sens)  # every row against its own sens and value
    print(f"{label}: dev/sens elpd_loo {q['elpd_loo']:.3g} pareto_k {q['pareto_k']:.3g} "
          f"(k from {np.nanmin(ref['pareto_k']):.3g} to {np.nanmax(ref['pareto_k']):.3g})")
    assert got.tail_len == ref["tail_len"] and got.n_nonfinite == ref["n_nonfinite"]
    assert max(q.values()) <= L.FACTOR, q
    return q


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("shape", SHAPES)
def test_tail_exactly_and_k_and_elpd_inside_the_yardstick(gm, shape, family, dtype):
    """Per draw count (M = 5, 52, and a second and third slab of the product
    pass): the tail is, bit for bit, the M largest of -pointwise - max(-pointwise)
    in float64 (the product's C/D placement, the selection and the sort, without
    a tolerance); pareto_k and elpd_loo of every row differ from the
    transcription on the device's own pointwise matrix by at most
    16 sens + 2^-50 max(1, |value|), sens and value that row's."""
    N, D = shape
    worst = {}
    for S in _counts(gm):
        case = P.synth_case(N, D, family, dtype, S)
        got, pw, ref, sens = _device_and_reference(gm, _target(gm, case), case.theta.astype(dtype))
        assert got.n_draws == S and got.elpd_loo.shape == (N,) and got.pareto_k.shape == (N,)
        _assert_tail(got, pw)
        q = _assert_parity(got, ref, sens, f"{shape} {family} {np.dtype(dtype).name} S={S}")
        for n, v in q.items():
            worst[n] = max(worst.get(n, 0.0), v)
        assert got.lppd.tobytes() == _target(gm, case).predict(case.theta.astype(dtype)).lppd.tobytes()
    print(f"{shape} {family} {np.dtype(dtype).name}: worst dev/sens {worst}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S,N", [(120000, 3), ((1 << 20) + 5, 2)])
def test_large_tails(gm, S, N, dtype):
    """M = 1040 (more values than the workgroup has threads, 2048 sort slots)
    and M = 3073 (4096 slots): the sort has one path for every M, so there is
    no size switch to straddle."""
    case = P.synth_case(N, 3, "poisson_log", dtype, S)
    got, pw, ref, sens = _device_and_reference(gm, _target(gm, case), case.theta.astype(dtype))
    assert got.tail_len == L.tail_len(S) > 1024
    _assert_tail(got, pw)
    _assert_parity(got, ref, sens, f"large tail S={S} {np.dtype(dtype).name}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_small_reff_gives_a_fifth_of_the_draws(gm, dtype):
    """reff = 0.01 at S = 8000: M = floor(0.2 S) = 1600, the longest tail S allows."""
    case = P.synth_case(3, 3, "bernoulli_logit", dtype, 8000)
    got, pw, ref, sens = _device_and_reference(gm, _target(gm, case), case.theta.astype(dtype), reff=0.01)
    assert got.tail_len == 1600
    _assert_tail(got, pw, 0.01)
    _assert_parity(got, ref, sens, f"reff 0.01 {np.dtype(dtype).name}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_row_groups(gm, family, dtype):
    """A workspace that holds 64 rows (two groups for 70 rows) against the
    default (one group of 128): every output bit for bit."""
    N, D = 70, 33
    S = 2 * gm.stats.predict_plan()["slab_draws"] + 15
    case = P.synth_case(N, D, family, dtype, S)
    t, th = _target(gm, case), case.theta.astype(dtype)
    one = gm.stats.loo_plan(dtype, S, N)
    assert one["group_rows"] == 128
    ws = 64 * one["row_bytes"] + one["row_bytes"] // 2
    assert gm.stats.loo_plan(dtype, S, N, workspace_bytes=ws)["group_rows"] == 64
    _bits(t.loo(th, tail=True), t.loo(th, tail=True, workspace_bytes=ws))


@pytest.mark.parametrize("dtype", DTYPES)
def test_repeatable_and_row_permutation(gm, dtype):
    N, D, S = 70, 33, 300
    case = P.synth_case(N, D, "poisson_log", dtype, S)
    th = case.theta.astype(dtype)
    a = _target(gm, case).loo(th, tail=True)
    _bits(a, _target(gm, case).loo(th, tail=True))
    perm = np.random.default_rng(2).permutation(N)
    b = gm.GLM(case.X[perm], case.y[perm], family="poisson_log", offset=case.off[perm]).loo(th, tail=True)
    _bits(a, b, perm)
    assert len({v for v in a.elpd_loo}) == N  # the rows differ


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_device_samples_of_a_run(gm, family, dtype):
    """The draws of a short HMC run, used where they lie, against the same
    draws passed from the host in stored order: bit for bit."""
    N, D, chains = 70, 33, 6
    X, y, off = R.synth(N, D, family, 3)
    r = lambda v: np.asarray(v, dtype=dtype).astype(np.float64)
    target = gm.GLM(r(X), r(y), family=family, prior_sd=2.0, offset=r(off))
    x0 = (0.1 * np.random.default_rng(5).standard_normal((chains, D))).astype(dtype)
    s = gm.HMC(target, x0, 0.02, 5, dtype=dtype).set_seed(9)
    ds = s.run_positions(20, 10)
    host = np.ascontiguousarray(ds.to_host().transpose(1, 0, 2))  # stored order [n_collect, n_chains, dim]
    a = target.loo(ds, tail=True)
    assert a.n_draws == 20 * chains and a.tail_len == L.tail_len(120)
    _bits(a, target.loo(host, tail=True))
    _assert_tail(a, target.predict(ds, pointwise=True).pointwise)
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_reversed_draws(gm, family, dtype):
    """The result is a function of the multiset of draws: reversed, the tail is
    bit for bit the same, pareto_k and elpd_loo stay inside the yardstick."""
    N, D = 70, 33
    S = gm.stats.predict_plan()["slab_draws"] + 1
    case = P.synth_case(N, D, family, dtype, S)
    t, th = _target(gm, case), case.theta.astype(dtype)
    got, pw, ref, sens = _device_and_reference(gm, t, th)
    rev = t.loo(np.ascontiguousarray(th[::-1]), tail=True)
    assert rev.tail.tobytes() == got.tail.tobytes()
    _assert_parity(rev, ref, sens, f"reversed {family} {np.dtype(dtype).name}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_rows(gm, dtype):
    """Poisson with one draw scaled until exp(eta) overflows in some rows: those
    rows are NaN and counted, every other row is finite and inside the
    yardstick. A NaN coefficient takes every row."""
    N, D, S = 17, 5, 300
    case = P.synth_case(N, D, "poisson_log", dtype, S)
    t = _target(gm, case)
    th = case.theta.astype(dtype)
    th[7] *= 1.0e4
    got, pw, ref, sens = _device_and_reference(gm, t, th)
    hit = ~np.all(np.isfinite(pw), axis=0)
    assert 0 < hit.sum() < N and np.all(np.isneginf(pw[7, hit])) and got.n_nonfinite == hit.sum()
    assert np.all(np.isnan(got.elpd_loo[hit])) and np.all(np.isnan(got.pareto_k[hit]))
    assert np.all(np.isnan(got.tail[hit])) and np.all(np.isfinite(got.tail[~hit]))
    # (the scaled draw dominates most of the other rows: x* = 0 there and pareto_k = +inf by the rule)
    assert np.all(np.isfinite(got.elpd_loo[~hit])) and not np.any(np.isnan(got.pareto_k[~hit]))
    assert np.any(np.isfinite(got.pareto_k[~hit])) and np.any(np.isposinf(got.pareto_k[~hit]))
    assert np.ascontiguousarray(got.tail[~hit]).tobytes() == L.raw_tail(pw[:, ~hit]).tobytes()
    _assert_parity(got, ref, sens, f"-inf rows {np.dtype(dtype).name}")
    assert list(got.bad_rows) == list(np.flatnonzero(np.nan_to_num(ref["pareto_k"], nan=-1.0) > got.k_threshold))
    th[11, 2] = np.nan
    every = t.loo(th, tail=True)
    assert every.n_nonfinite == N and np.all(np.isnan(every.elpd_loo)) and np.all(np.isnan(every.pareto_k))
    assert np.all(np.isnan(every.tail)) and every.n_bad_k == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S", [1, 4, 24, 25])
def test_small_draw_counts(gm, S, dtype):
    """Below M = 5 (S < 25) nothing is fitted: k = +inf and elpd_loo is the raw
    importance-sampling value; S = 1 gives ll itself; S = 25 fits."""
    case = P.synth_case(17, 5, "bernoulli_logit", dtype, S)
    got, pw, ref, sens = _device_and_reference(gm, _target(gm, case), case.theta.astype(dtype).reshape(S, 5))
    assert got.tail_len == [0, 0, 4, 5][[1, 4, 24, 25].index(S)]
    _assert_tail(got, pw)
    if S < 25:
        assert np.all(got.pareto_k == np.inf) and got.n_bad_k == 17
        raw = L.loo(pw, smooth=False)
        assert np.array_equal(raw["elpd_loo"], ref["elpd_loo"])
    else:
        assert np.all(np.isfinite(got.pareto_k))
    if S == 1:
        assert got.elpd_loo.tobytes() == pw[0].astype(np.float64).tobytes()
    _assert_parity(got, ref, sens, f"S={S} {np.dtype(dtype).name}")


def test_an_influential_row(gm):
    """A 70 x 3 logistic fit by NUTS, 64 chains x 300 draws; row 0 has x = 6 and
    y = 0. It has the largest pareto_k; p_loo and the distance to WAIC are in
    loose sanity bands around what the transcription gave on Laplace draws
    (p_loo 3.25, difference 0.05)."""
    rng = np.random.default_rng(0)
    N, D = 70, 3
    X = np.column_stack([np.ones(N), rng.normal(size=(N, D - 1))])
    y = (rng.random(N) < 1.0 / (1.0 + np.exp(-X @ np.array([0.3, 1.0, -0.7])))).astype(np.float64)
    X[0, 1], y[0] = 6.0, 0.0
    target = gm.GLM(X, y, prior_sd=2.0)
    x0 = 0.1 * gm.init_with_seed(64, D, 3, np.float64)
    s = gm.NUTS.new_with_mass_matrix(target, x0, 0.8, gm.NUTSMassMatrixConfig(), dtype=np.float64).set_seed(5)
    ds = s.run_positions(300, 200)
    loo = target.loo(ds)
    waic = target.predict(ds).waic()
    print(loo)
    print(waic)
    print(f"row 0: k {loo.pareto_k[0]:.3f}, the rest at most {np.max(loo.pareto_k[1:]):.3f}; p_loo {loo.p_loo:.3f}")
    assert loo.n_draws == 64 * 300 and loo.n_nonfinite == 0 and loo.tail is None
    assert int(np.argmax(loo.pareto_k)) == 0
    assert 1.0 < loo.p_loo < 10.0
    assert abs(loo.elpd_loo_sum - waic.elpd_waic) < 1.0
    assert loo.looic == -2.0 * loo.elpd_loo_sum and loo.se > 0
    s.close()


def test_refusals(gm):
    """Each refusal names its argument."""
    case = P.synth_case(17, 5, "bernoulli_logit", np.float64, 300)
    t = _target(gm, case)
    for reff in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="reff"):
            t.loo(case.theta, reff=reff)
    with pytest.raises(gm.GMError, match="workspace_bytes = 4096 is too small: 64 rows of 300 draws need"):
        t.loo(case.theta, workspace_bytes=4096)
    with pytest.raises(ValueError, match="dim = 5"):
        t.loo(np.zeros((300, 4)))
    with pytest.raises(gm.GMError, match="n_draws must be <= 2\\^24"):
        gm.stats.loo_plan(np.float32, (1 << 24) + 1, 17)
    with pytest.raises(gm.GMError, match="n_rows must be <= 2\\^24"):
        gm.stats.loo_plan(np.float32, 300, (1 << 24) + 1)
    # the C entry points: a model without y, dim out of range
    import ctypes as C
    lib = gm._lib.load()
    dp = C.POINTER(C.c_double)
    desc = gm._lib.gm_glm_desc()
    desc.family, desc.n_rows, desc.x = 1, 17, t.X.ctypes.data_as(dp)
    out = gm._lib.gm_glm_loo_out()
    th = np.ascontiguousarray(case.theta)
    assert lib.gm_glm_loo(C.byref(desc), 5, gm._lib.GM_F64, gm._lib.ptr(th), 300, 1.0, 0,
                          C.byref(out)) == gm._lib.GM_EINVAL
    assert b"y must not be NULL" in lib.gm_last_error()
    desc.y = t.y.ctypes.data_as(dp)
    assert lib.gm_glm_loo(C.byref(desc), 129, gm._lib.GM_F64, gm._lib.ptr(th), 300, 1.0, 0,
                          C.byref(out)) == gm._lib.GM_EINVAL
    assert b"dim must be in [1, 128]" in lib.gm_last_error()
