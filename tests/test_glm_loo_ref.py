"""The GLM PSIS-LOO without a GPU: the float64 transcription
(tests/_glm_loo_ref.py) on exact generalised Pareto samples, its edge semantics,
the multiset property, Jensen's inequality, GLMLoo's arithmetic, the plan and
every refusal of the C ABI (validation runs before the first device call)."""
import ctypes as C

import numpy as np
import pytest

from tests import _glm_loo_ref as L
from tests import _glm_predict_ref as P
from tests import _glm_ref as R


def _ll(M=17, D=5, family="bernoulli_logit", S=300):
    return P.pointwise(P.synth_case(M, D, family, np.float64, S))[3]


@pytest.mark.parametrize("k,seen", [(0.1, 0.100), (0.5, 0.491), (0.9, 0.954)])
def test_gpd_recovery(k, seen):
    """Exact GPD(k, sigma = 1) samples, n = 3000: k-hat before the prior step is
    within 0.1 of k (0.100, 0.491, 0.954 when this was written)."""
    u = np.random.default_rng(0).random((3, 3000))[[0.1, 0.5, 0.9].index(k)]
    x = np.sort(np.expm1(-k * np.log1p(-u)) / k)
    kh, sigma = L.gpdfit(x, prior=False)
    print(f"k = {k}: k-hat {kh:.4f}, sigma-hat {sigma:.4f}")
    assert abs(kh - k) < 0.1 and abs(sigma - 1.0) < 0.2
    kp, _ = L.gpdfit(x)
    assert kp == (kh * 3000 + 5.0) / 3010.0
    kf, _ = L.gpdfit(x, L.Ops(1), prior=False)
    assert kf != kh and abs(kf - kh) < 1e-9


def test_tail_length_and_threshold():
    assert [L.tail_len(S) for S in (1, 4, 5, 24, 25, 300, 4096000, 1 << 24)] == [0, 0, 1, 4, 5, 52, 6072, 12288]
    assert L.tail_len(1000, 0.01) == 200 and L.tail_len(1000, 4.0) == 48
    assert L.k_threshold(100) == 0.5 and L.k_threshold(4096000) == 0.7 and L.k_threshold(1) == -np.inf


def test_small_draw_counts():
    """S = 1: elpd_loo = ll_1, k = +inf. S = 24 (M = 4): no fit, the raw
    importance-sampling value. S = 25 (M = 5): a fit."""
    ll = _ll(S=25)
    e, k, t = L.psis_row(ll[:1, 0])
    assert e == ll[0, 0] and k == np.inf and t.size == 0
    e, k, t = L.psis_row(ll[:24, 0])
    raw = -(np.log(np.mean(np.exp(-(ll[:24, 0] - ll[:24, 0].min())))) - ll[:24, 0].min())
    assert k == np.inf and t.size == 4 and abs(e - raw) < 1e-13 * max(1.0, abs(raw))
    assert L.psis_row(ll[:24, 0], smooth=False)[0] == e
    e, k, t = L.psis_row(ll[:, 0])
    assert np.isfinite(k) and t.size == 5 and np.isfinite(e)
    assert np.array_equal(t, np.sort(-ll[:, 0] - np.max(-ll[:, 0]))[-5:])


def test_equal_draws():
    e, k, t = L.psis_row(np.full(300, -1.25))
    assert k == np.inf and e == -1.25 and np.all(t == 0.0)


@pytest.mark.parametrize("bad", [-np.inf, np.inf, np.nan])
def test_a_non_finite_entry_takes_its_row_only(bad):
    ll = _ll()
    ref = L.loo(ll)
    ll2 = ll.copy()
    ll2[7, 3] = bad
    got = L.loo(ll2)
    assert got["n_nonfinite"] == 1 and ref["n_nonfinite"] == 0
    assert np.isnan(got["elpd_loo"][3]) and np.isnan(got["pareto_k"][3]) and np.all(np.isnan(got["tail"][3]))
    keep = np.arange(17) != 3
    for n in ("elpd_loo", "pareto_k", "tail"):
        assert np.array_equal(got[n][keep], ref[n][keep]), n


@pytest.mark.parametrize("family", R.FAMILIES)
def test_the_result_depends_on_the_multiset_of_draws(family):
    """Permuting the draws: the same tail, k and elpd_loo inside the yardstick."""
    ll = _ll(family=family, S=300)
    ref = L.loo(ll)
    sens = L.sensitivity(ll, plain=ref)
    perm = np.random.default_rng(4).permutation(300)
    got = L.loo(ll[perm])
    assert np.array_equal(got["tail"], ref["tail"])
    q = L.ratios(got, ref, sens)
    print(f"{family}: permuted / yardstick {q}")
    assert max(q.values()) <= L.FACTOR
    assert np.array_equal(L.raw_tail(ll), ref["tail"])


@pytest.mark.parametrize("family", R.FAMILIES)
def test_jensen(family):
    """The raw importance-sampling elpd_loo is the log of a harmonic mean: <= lppd."""
    ll = _ll(70, 33, family, 300)
    raw = L.loo(ll, smooth=False)
    lppd = P.lppd_of(ll)
    assert np.all(raw["pareto_k"] == np.inf)
    assert np.all(raw["elpd_loo"] <= lppd + 1e-12 * np.maximum(1.0, np.abs(lppd)))
    sm = L.loo(ll)
    assert np.all(np.isfinite(sm["pareto_k"])) and np.all(np.isfinite(sm["elpd_loo"]))


def test_glmloo_scalars():
    import general_mcmc_amd as gm
    elpd = np.array([-1.0, -2.5, -0.5])
    k = np.array([0.2, np.inf, 0.69])
    lppd = np.array([-0.9, -2.0, -0.45])
    r = gm.GLMLoo(elpd, k, lppd, None, 52, 0, 300)
    assert r.elpd_loo_sum == -4.0 and r.looic == 8.0
    assert abs(r.p_loo - 0.65) < 1e-15
    assert r.se == float(np.sqrt(3 * np.var(elpd, ddof=1)))
    assert r.k_threshold == min(1.0 - 1.0 / np.log10(300.0), 0.7) and r.k_threshold < 0.6
    assert r.n_bad_k == 2 and list(r.bad_rows) == [1, 2]
    assert "elpd_loo" in str(r) and "2 of 3 rows have a Pareto k above" in str(r)
    big = gm.GLMLoo(elpd, np.array([0.2, np.nan, 0.69]), lppd, None, 6072, 1, 4096000)
    assert big.k_threshold == 0.7 and big.n_bad_k == 0 and "1 rows have a non-finite" in str(big)
    assert np.isnan(gm.GLMLoo(elpd[:1], k[:1], lppd[:1], None, 0, 0, 1).se)


def test_plan():
    import general_mcmc_amd as gm
    p = gm.stats.loo_plan(np.float32, 4096000, 1024)
    assert p["tail_len"] == 6072 and p["sort_slots"] == 8192 and p["max_draws"] == 1 << 24
    assert p["default_workspace_bytes"] == (1 << 32) + (1 << 28) and p["group_rows"] % 64 == 0 and p["group_rows"] >= 64
    assert p["row_bytes"] == 4096000 * 4 + 2 * 8192 * 8 + 20
    assert p["workspace_bytes"] == p["group_rows"] * p["row_bytes"] <= (1 << 32) + (1 << 28)
    assert gm.stats.loo_plan(np.float32, 300, 70)["group_rows"] == 128
    one = gm.stats.loo_plan(np.float64, 300, 70, workspace_bytes=64 * (300 * 8 + 2 * 64 * 8 + 20))
    assert one["group_rows"] == 64 and one["tail_len"] == 52
    assert gm.stats.loo_plan(np.float64, 1 << 24, 64, workspace_bytes=1 << 34)["tail_len"] == 12288
    assert gm.stats.loo_plan(np.float32, 1000, 1, reff=0.01)["tail_len"] == 200
    # [5]: the largest draw count of which the dtype and the workspace hold 64 rows
    f64 = gm.stats.loo_plan(np.float64, 300, 70)["max_draws"]
    assert 8_800_000 < f64 < 8_900_000
    assert gm.stats.loo_plan(np.float64, f64, 70)["group_rows"] == 64
    with pytest.raises(gm.GMError, match=f"up to {f64} draws"):
        gm.stats.loo_plan(np.float64, f64 + 1, 70)
    assert gm.stats.loo_plan(np.float64, 300, 70, workspace_bytes=1 << 34)["max_draws"] == 1 << 24
    assert gm.stats.loo_plan(np.float64, 300, 70, workspace_bytes=64 * (300 * 8 + 2 * 64 * 8 + 20))["max_draws"] == 300


def test_refusals():
    """Each GM_EINVAL of gm_glm_loo / gm_glm_loo_device / gm_glm_loo_plan names its argument."""
    import general_mcmc_amd as gm
    lib = gm._lib.load()
    dp = C.POINTER(C.c_double)
    X, y = np.ones((4, 3)), np.zeros(4)
    th = np.zeros((5, 3))
    e, k = np.empty(4), np.empty(4)

    def call(X=X, y=y, dim=3, n_rows=4, draws=th, n_draws=5, reff=1.0, ws=0, device=False, family=1, out=True):
        d = gm._lib.gm_glm_desc()
        d.family, d.n_rows = family, n_rows
        d.x = X.ctypes.data_as(dp) if X is not None else None
        d.y = y.ctypes.data_as(dp) if y is not None else None
        o = gm._lib.gm_glm_loo_out(elpd_loo=e.ctypes.data, pareto_k=k.ctypes.data)
        op = C.byref(o) if out else None
        dr = gm._lib.ptr(draws) if draws is not None else None
        if device:
            rc = lib.gm_glm_loo_device(C.byref(d), dim, gm._lib.GM_F64, dr, n_draws, dim, reff, ws, op)
        else:
            rc = lib.gm_glm_loo(C.byref(d), dim, gm._lib.GM_F64, dr, n_draws, reff, ws, op)
        return rc, lib.gm_last_error().decode()

    for kw, word in (({"y": None}, "y must not be NULL"), ({"reff": 0.0}, "reff"), ({"reff": -1.0}, "reff"),
                     ({"reff": np.inf}, "reff"), ({"reff": np.nan}, "reff"), ({"dim": 0}, "dim must be in [1, 128]"),
                     ({"dim": 129}, "dim must be in [1, 128]"), ({"n_rows": 0}, "n_rows must be >= 1"),
                     ({"n_rows": (1 << 24) + 1}, "n_rows must be <= 2^24"), ({"ws": 1000}, "workspace_bytes = 1000"),
                     ({"ws": -1}, "workspace_bytes"), ({"n_draws": 0}, "n_draws must be >= 1"),
                     ({"n_draws": (1 << 24) + 1}, "n_draws must be <= 2^24"), ({"draws": None}, "draws is NULL"),
                     ({"X": None}, "x must not be NULL"), ({"family": 3}, "family"), ({"out": False}, "out is NULL"),
                     ({"y": np.array([0.0, 2.0, 0.0, 0.0])}, "0 <= y <= 1 at row 1"),
                     ({"X": np.array([[1.0] * 3] * 3 + [[1.0, np.nan, 1.0]])}, "x is not finite at row 3, column 1")):
        for device in (False, True):
            rc, msg = call(device=device, **kw)
            assert rc == gm._lib.GM_EINVAL and word in msg, (kw, device, msg)
    rc, msg = call(ws=1000)
    assert "64 rows of 5 draws need " + str(64 * (8 * 8 + 2 * 2 * 8 + 20)) + " bytes" in msg
    v = (C.c_int64 * 7)()
    assert lib.gm_glm_loo_plan(gm._lib.GM_F64, 5, 4, 1.0, 0, None, 7) == gm._lib.GM_EINVAL
    assert lib.gm_glm_loo_plan(gm._lib.GM_F64, 5, 4, 0.0, 0, v, 7) == gm._lib.GM_EINVAL
    assert b"reff" in lib.gm_last_error()
    assert lib.gm_glm_loo_plan(7, 5, 4, 1.0, 0, v, 7) == gm._lib.GM_EINVAL
    for n in ("gm_glm_loo", "gm_glm_loo_device", "gm_glm_loo_plan"):
        assert hasattr(lib, n)
    assert C.sizeof(gm._lib.gm_glm_loo_out) == 3 * C.sizeof(C.c_void_p) + 16


def test_facade_refusals_before_any_device_work():
    import general_mcmc_amd as gm
    t = gm.GLM(np.ones((4, 3)), np.zeros(4))
    for reff in (0.0, -2.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="reff"):
            t.loo(np.zeros((5, 3)), reff=reff)
    with pytest.raises(gm.GMError, match="workspace_bytes = 1000 is too small"):
        t.loo(np.zeros((5, 3)), workspace_bytes=1000)
    with pytest.raises(ValueError, match="dim = 3"):
        t.loo(np.zeros((5, 4)))
    with pytest.raises(ValueError, match="no draws"):
        t.loo(np.zeros((0, 3)))
