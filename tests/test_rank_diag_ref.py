"""The posterior summary's definitions (tests/_rank_diag_ref.py, the checker
of the GPU tests) on hand cases and on draws with known behaviour, plus the
parts of the new C ABI that need no GPU: argument validation (every GM_EINVAL
is returned before any device call) and the exported names."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from scipy.special import ndtri

from tests import _rank_diag_ref as ref
from tests._diag_cases import exact_f64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gm_summary", "gm_summary_device", "gm_rank_normalize", "gm_summary_sort_plan"]


def test_hand_ranks_and_scores():
    y = np.array([[3.0, 1.0], [2.0, 2.0]], dtype=np.float32)
    r, z = ref.ranks_of(y)
    np.testing.assert_array_equal(r.reshape(-1), [4.0, 1.0, 2.5, 2.5])
    np.testing.assert_array_equal(z, ndtri((r - 0.375) / 4.25))
    assert z[1, 0] == z[1, 1] and z[0, 1] == -z[0, 0]
    # -0.0 and +0.0 tie; f64 values below f32 resolution do not
    r, _ = ref.ranks_of(np.array([[-0.0, 0.0], [1.0, -1.0]]))
    np.testing.assert_array_equal(r.reshape(-1), [2.5, 2.5, 4.0, 1.0])
    r, _ = ref.ranks_of(np.array([[1.0, 1.0 + 2.0 ** -40], [1.0 - 2.0 ** -40, 1.0]]))
    np.testing.assert_array_equal(r.reshape(-1), [2.5, 4.0, 1.0, 2.5])


def test_order_statistic_indices():
    # (M - 1) q near an integer: M = 41 -> 40 * 0.05 = 2 (exactly 2.0 in f64),
    # M = 21 -> 20 * 0.95 = 19 exactly, M = 40 -> 39 * 0.05 = 1.95
    assert ref.order_index(40, 0.05) == 1 and ref.order_index(40, 0.95) == 37
    assert ref.order_index(41, 0.05) == 2 and ref.order_index(41, 0.95) == 38
    assert ref.order_index(21, 0.95) == 19 and ref.order_index(61, 0.05) == 3
    for m in (40, 41, 280, 65920, 1050624):
        for q in (0.05, 0.95):
            k = ref.order_index(m, q)
            assert 0 <= k <= m - 1 and k <= (m - 1) * q < k + 1


def test_split_of_odd_draw_count():
    x = np.arange(2 * 7, dtype=np.float64).reshape(2, 7, 1)
    y = ref.split(x[:, :, 0])
    np.testing.assert_array_equal(y, [[0, 1, 2], [7, 8, 9], [4, 5, 6], [11, 12, 13]])
    rk, z = ref.rank_normalize(x)
    assert np.isnan(rk[:, 3, 0]).all() and np.isnan(z[:, 3, 0]).all()
    assert np.isfinite(np.delete(rk, 3, axis=1)).all()
    np.testing.assert_array_equal(np.sort(rk[np.isfinite(rk)]), np.arange(1, 13))
    rf, _ = ref.rank_normalize(x, folded=True)  # |y - 6.5|: symmetric pairs tie
    assert rf[0, 0, 0] == rf[1, 6, 0] == 11.5


def test_appb_is_the_project_estimator():
    rng = np.random.default_rng(3)
    x = (np.cumsum(rng.standard_normal((6, 80, 2)), axis=1) * 0.2 + rng.standard_normal((6, 80, 2))).astype(np.float32)
    xr, xe = exact_f64(x)
    for p in range(2):
        r, e, margin = ref.appb(ref.split(x[:, :, p]))
        np.testing.assert_allclose([r, e], [xr[p], xe[p]], rtol=1e-10)
        assert margin > 0


def test_iid_normal_draws():
    x = np.random.default_rng(11).standard_normal((8, 500, 3))
    s = ref.summary(x)
    m = 8 * 500
    assert (s["rhat"] < 1.01).all() and (s["rhat"] >= 0.999).all()
    assert (np.abs(s["ess_bulk"] - m) < 0.15 * m).all()
    np.testing.assert_allclose(s["mean"], x.mean(axis=(0, 1)), rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(s["quantiles"][1], np.median(x.reshape(-1, 3), axis=0), rtol=1e-13)


def test_shifted_chain_raises_rhat():
    # One of C chains shifted by d = 1 sigma: 2 of the 2C split-chain means are
    # off by d, so B / h ~ d^2 (1/C)(1 - 1/C) 2C / (2C - 1) and, with W ~ 1,
    # rhat ~ sqrt(1 + B / (h W)): 1.057 for C = 8, 1.10 for C = 4, 1.155 for C = 2.
    x = np.random.default_rng(12).standard_normal((2, 500, 1))
    x[0] += 1.0
    assert ref.summary(x)["rhat"][0] > 1.1
    x = np.random.default_rng(12).standard_normal((8, 500, 1))
    x[0] += 1.0
    assert 1.04 < ref.summary(x)["rhat"][0] < 1.08


def test_scaled_chain_shows_in_folded_rhat():
    x = np.random.default_rng(13).standard_normal((8, 500, 1))
    x[0] *= 3.0
    s = ref.summary(x)
    assert s["rhat_fold"][0] > s["rhat_bulk"][0] and s["rhat"][0] == s["rhat_fold"][0]


def test_degenerate_parameters():
    x = np.random.default_rng(14).standard_normal((4, 20, 3))
    x[:, :, 1] = 2.5
    x[1, 3, 2] = np.nan
    s = ref.summary(x)
    assert np.isfinite(s["rhat"][0])
    assert s["mean"][1] == 2.5 and (s["quantiles"][:, 1] == 2.5).all()
    assert np.isnan([s["rhat"][1], s["ess_bulk"][1], s["ess_tail"][1]]).all()
    assert np.isnan([s[k][2] for k in ("mean", "sd", "rhat", "ess_bulk", "ess_tail")]).all()
    assert np.isnan(s["quantiles"][:, 2]).all()


def test_generator_kinds():
    for kind in ref.KINDS:
        a = ref.generate(kind, (4, 50, 2), np.float32)
        assert a.dtype == np.float32 and a.shape == (4, 50, 2) and np.isfinite(a).all()
        np.testing.assert_array_equal(a, ref.generate(kind, (4, 50, 2), np.float32))
    t = ref.generate("ties", (4, 200, 2), np.float64)
    rep = (t[:, 1:] == t[:, :-1]).mean()
    assert 0.55 < rep < 0.75


# ---- the C ABI, without a GPU ---------------------------------------------------

def _lib():
    import general_mcmc_amd as g
    return g, g._lib.load()


def test_new_header_symbols_exported():
    g, lib = _lib()
    src = open(os.path.join(ROOT, "include", "gmcmc.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\b(gm_[a-z0-9_]+)\s*\(", src))
    for n in NEW:
        assert n in names, f"{n} not declared in gmcmc.h"
        assert hasattr(lib, n), f"{n} declared in gmcmc.h but not exported"
        assert n in g._lib.SIGNATURES
    for n in ("Summary", "summary", "rank_normalize"):
        assert n in g.__all__ and hasattr(g, n)


def test_sort_plan_readback():
    g, lib = _lib()
    v = (C.c_int32 * 4)(-1, -1, -1, -1)
    assert lib.gm_summary_sort_plan(v, 3) == g._lib.GM_OK
    assert v[0] >= 64 and v[1] >= 64 and 1 <= v[2] <= 16 and v[3] == -1
    assert lib.gm_summary_sort_plan(None, 3) == g._lib.GM_EINVAL
    assert g.stats.sort_plan()["lds_max"] == v[0]


def test_argument_validation_needs_no_device():
    g, lib = _lib()
    L = g._lib
    x = np.zeros((2, 8, 3), dtype=np.float32)
    f = {n: np.empty(3) for n in ("mean", "sd", "rhat", "ess_bulk", "ess_tail")}
    f["quantiles"] = np.empty((2, 3))
    out = L.gm_summary_out(**{n: a.ctypes.data for n, a in f.items()})
    probs = np.array([0.1, 0.9])
    pp, po, px = L.ptr(probs), C.byref(out), L.ptr(x)

    def host(sample=px, dt=L.GM_F32, c=2, n=8, p=3, k=2, pr=pp, o=po):
        return lib.gm_summary(sample, dt, c, n, p, k, pr, o)

    def dev(sample=px, dt=L.GM_F32, c=2, n=8, p=3, k=2, pr=pp, o=po):
        return lib.gm_summary_device(sample, dt, c, n, p, 24, 3, 1, k, pr, o)

    def rk(sample=px, dt=L.GM_F32, c=2, n=8, p=3):
        r = np.empty((2, 8, 3))
        return lib.gm_rank_normalize(sample, dt, c, n, p, 0, L.ptr(r), None)

    bad_pr = [np.array([0.5, 1.5]), np.array([-0.1, 0.5]), np.array([np.nan, 0.5])]
    for fn in (host, dev):
        cases = [dict(dt=7), dict(sample=None), dict(o=None), dict(c=0), dict(n=3), dict(p=0), dict(k=-1),
                 dict(k=33), dict(c=1 << 20, n=1 << 12)] + [dict(pr=L.ptr(b)) for b in bad_pr]
        for kw in cases:
            assert fn(**kw) == L.GM_EINVAL, kw
            assert lib.gm_last_error()
    for kw in (dict(dt=7), dict(sample=None), dict(c=0), dict(n=3), dict(p=0), dict(c=1 << 20, n=1 << 12)):
        assert rk(**kw) == L.GM_EINVAL, kw
    # M = 2^31 - 2 is the largest pooled count let through to the device stage; 2^31 is refused
    assert host(c=1 << 20, n=1 << 11) == L.GM_EINVAL
    with pytest.raises(ValueError):
        g.summary(np.zeros((3, 4)))
