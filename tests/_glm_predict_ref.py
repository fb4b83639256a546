"""A numpy float64 reference of the GLM posterior prediction (include/gmcmc.h
gm_glm_predict, glm_predict_device.h) and the derived bounds that the GPU tests
hold the device to.

Per draw s and row m:
    eta = offset_m + sum_j X[m][j] theta_sj
    mu  = logistic(eta) | exp(eta)
    ll  = (y_m eta - A(eta)) + c_m,   c_m = -lgamma(y_m + 1) (Poisson) | 0
Per row, over the S draws: mean / sd (ddof = 1) of eta and mu, mean / variance
(ddof = 1) of ll, lppd = log((1/S) sum_s exp ll) by the maximum-shifted sum.

Bounds, u the unit roundoff of the draws' dtype, k = 8 (D + 1) u,
a = |theta| |x| + |offset|:
    |d eta| <= k a
    |d mu|  <= mu (k a + k)
    |d ll|  <= k (|y eta| + |A| + (|y| + mu) a + |c|)
    tau_m = max_s of the ll bound: |d lppd| <= tau, |d ll_var| <= 2 sd_ll tau' + tau'^2,
    tau' = tau sqrt(S / (S - 1))
    means: the mean of the per-draw bounds; sds: the largest per-draw bound times sqrt(S / (S - 1))
and every reduced output also S 2^-53 times the sum of the absolute values of
the terms it sums (the float64 accumulation).
"""
import math

import numpy as np

from tests import _glm_ref as R

# (M, D) of the GPU tests, each the smallest that reaches its path: one row; a
# partial row tile with D no multiple of 4 (2 k-steps of 4 columns); a second,
# partial workgroup tile at 16 k-steps, one column past a multiple of 4; the
# 32-k-step instantiation; five workgroup tiles. (33, 20) is the 8-k-step
# instantiation, which none of the others reaches.
SHAPES = [(1, 1), (17, 5), (70, 33), (70, 128), (300, 64), (33, 20)]
OUTPUTS = ("eta_mean", "eta_sd", "mu_mean", "mu_sd", "lppd", "ll_mean", "ll_var")
ACC = 2.0 ** -53


def draw_counts(slab):
    """1; a partial matrix-core tile; 300; a second slab of one draw; two slabs and a partial tile."""
    return [1, 15, 300, slab + 1, 2 * slab + 15]


def lgamma1(y):
    return np.array([math.lgamma(v + 1.0) for v in np.asarray(y, dtype=np.float64).reshape(-1)])


class Case:
    """A model and draws as the device holds them: everything rounded to dtype, then float64."""

    def __init__(self, X, y, off, family, theta, dtype):
        r = lambda v: np.asarray(v, dtype=np.float64).astype(dtype).astype(np.float64)
        self.family, self.dtype = family, np.dtype(dtype)
        self.X = r(X)
        self.M, self.D = self.X.shape
        self.off = np.zeros(self.M) if off is None else r(off)
        self.y = None if y is None else r(y)
        self.theta = r(theta).reshape(-1, self.D)
        self.S = self.theta.shape[0]
        if self.y is None:
            self.c = None
        else:
            self.c = r(-lgamma1(self.y)) if family == "poisson_log" else np.zeros(self.M)
        self.glm = R.GlmRef(self.X, np.zeros(self.M) if self.y is None else self.y, family, 1.0, self.off)


def synth_case(M, D, family, dtype, S, seed=11):
    X, y, off = R.synth(M, D, family, 3)
    theta = 0.5 * np.random.default_rng(seed).standard_normal((S, D))
    return Case(X, y, off, family, theta, dtype)


def pointwise(case):
    """eta, mu, A [S, M] and ll (None without y), float64."""
    with np.errstate(over="ignore", invalid="ignore"):
        eta = case.theta @ case.X.T + case.off
        A, mu = case.glm.link(eta)
        ll = None if case.y is None else (case.y * eta - A) + case.c
    return eta, mu, A, ll


def lppd_of(ll):
    """log((1/S) sum_s exp ll) per column by the maximum-shifted sum; -inf where every entry is."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        m = np.max(ll, axis=0)  # (a NaN propagates)
        shifted = np.where(np.isneginf(m), 0.0, ll - np.where(np.isneginf(m), 0.0, m))
        v = m + np.log(np.mean(np.exp(shifted), axis=0))
        return np.where(np.isneginf(m), -np.inf, v)


def _mean_sd(x, var=False):
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        m = np.mean(x, axis=0)
        if x.shape[0] < 2:
            return m, np.full(x.shape[1], np.nan)
        v = np.var(x, axis=0, ddof=1)
        return m, (v if var else np.sqrt(v))


def reduce(eta, mu, ll):
    out = {}
    out["eta_mean"], out["eta_sd"] = _mean_sd(eta)
    out["mu_mean"], out["mu_sd"] = _mean_sd(mu)
    if ll is not None:
        out["ll_mean"], out["ll_var"] = _mean_sd(ll, var=True)
        out["lppd"] = lppd_of(ll)
    return out


def predict(case):
    """The seven per-row outputs (four without y) and the pointwise ll."""
    eta, mu, A, ll = pointwise(case)
    out = reduce(eta, mu, ll)
    out["pointwise"] = ll
    return out


def waic(lppd, ll_var):
    elpd = lppd - ll_var
    m = len(elpd)
    return {"elpd_waic": float(np.sum(elpd)), "p_waic": float(np.sum(ll_var)),
            "se": float(np.sqrt(m * np.var(elpd, ddof=1))), "waic": -2.0 * float(np.sum(elpd)), "pointwise": elpd,
            "n_high_variance": int(np.sum(ll_var > 0.4))}


def bounds(case):
    """The bounds of the module's docstring: a dict over OUTPUTS and "pointwise" ([S, M])."""
    u = R.unit_roundoff(case.dtype)
    k = 8.0 * (case.D + 1) * u
    S = case.S
    eta, mu, A, ll = pointwise(case)
    a = np.abs(case.theta) @ np.abs(case.X).T + np.abs(case.off)
    infl = math.sqrt(S / (S - 1.0)) if S > 1 else np.nan
    with np.errstate(over="ignore", invalid="ignore"):
        b_eta = k * a
        b_mu = mu * (k * a + k)
        b = {"eta_mean": np.mean(b_eta, axis=0) + ACC * np.sum(np.abs(eta), axis=0),
             "mu_mean": np.mean(b_mu, axis=0) + ACC * np.sum(np.abs(mu), axis=0)}
        for name, x, bx in (("eta_sd", eta, b_eta), ("mu_sd", mu, b_mu)):
            sd = _mean_sd(x)[1]
            # the accumulation term of the variance, S 2^-53 var, through the square root
            b[name] = np.max(bx, axis=0) * infl + S * ACC * sd
        if ll is not None:
            b_ll = k * (np.abs(case.y * eta) + np.abs(A) + (np.abs(case.y) + mu) * a + np.abs(case.c))
            tau = np.max(b_ll, axis=0)
            var = _mean_sd(ll, var=True)[1]
            b["pointwise"] = b_ll
            b["ll_mean"] = np.mean(b_ll, axis=0) + ACC * np.sum(np.abs(ll), axis=0)
            b["lppd"] = tau + S * ACC  # the terms exp(ll - max) / sum are positive and sum to 1
            tp = tau * infl
            b["ll_var"] = 2.0 * np.sqrt(var) * tp + tp * tp + S * ACC * var
    return b


def emulate_f32(case):
    """The evaluation in float32 with a sequential sum and two roundings per term (no fma):
    eta, mu, ll [S, M] as float64 views of float32 values."""
    f = np.float32
    th, X = case.theta.astype(f), case.X.astype(f)
    eta = np.broadcast_to(case.off.astype(f), (case.S, case.M)).copy()
    for j in range(case.D):
        eta = (eta + (th[:, j:j + 1] * X[None, :, j]).astype(f)).astype(f)
    with np.errstate(over="ignore", invalid="ignore"):
        if case.family == "poisson_log":
            mu = np.exp(eta).astype(f)
            A = mu
        else:
            em = np.exp(-np.abs(eta)).astype(f)
            A = (np.maximum(eta, f(0)) + np.log1p(em).astype(f)).astype(f)
            mu = (np.where(eta >= 0, f(1), em) / (f(1) + em)).astype(f)
        ll = None
        if case.y is not None:
            ll = (((case.y.astype(f) * eta).astype(f) - A).astype(f) + case.c.astype(f)).astype(f)
    d = lambda v: None if v is None else v.astype(np.float64)
    return d(eta), d(mu), d(ll)


def ratios(got, ref, bnd, names):
    """max |got - ref| / bound per name; non-finite reference entries must match exactly."""
    out = {}
    for n in names:
        g, r, b = np.asarray(got[n], dtype=np.float64), np.asarray(ref[n]), np.asarray(bnd[n])
        fin = np.isfinite(r)
        assert np.array_equal(np.isnan(g), np.isnan(r)), f"{n}: NaN pattern differs"
        assert np.array_equal(g[~fin & ~np.isnan(r)], r[~fin & ~np.isnan(r)]), f"{n}: infinities differ"
        d = np.abs(g[fin] - r[fin])
        bb = b[fin]
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.where(d == 0, 0.0, d / bb)
        out[n] = float(np.max(q)) if q.size else 0.0
    return out
