"""NumPy / SciPy transcription of the posterior summary's definitions
(include/gmcmc.h, "posterior summary"): the checker of gm_summary and
gm_rank_normalize, and the host route timed by tools/summary_timing.py.

For X[c, t, p], h = N // 2, Y = concat_c(X[:, :h], X[:, N-h:]) ([2C, h]) and
M = 2 C h, per parameter:
  r         scipy.stats.rankdata(Y, "average") in the sample's own dtype
  z         ndtri((r - 3/8) / (M + 1/4))
  AppB(S)   SURVEY Appendix B on an already split series S[2C, h] (the
            formulas of tests/_diag_cases.exact_f64, autocovariances by FFT)
  ess_bulk  ESS(AppB(z));  rhat = max(1/R(AppB(z)), 1/R(AppB(z_fold))), z_fold
            the scores of |Y - median| formed in f64
  ess_tail  min over q in (0.05, 0.95) of ESS(AppB(I(Y <= y_(floor((M-1) q)))))
  quantiles np.quantile(Y, probs);  mean, sd (ddof = 1) over all C N draws
Test infrastructure only."""
from __future__ import annotations

import numpy as np
from scipy.special import ndtri
from scipy.stats import rankdata

KINDS = ("ar", "cauchy", "ties")


def generate(kind: str, shape, dtype, seed_shift: int = 0) -> np.ndarray:
    """x = cumsum(N(0,1), axis=1) * 0.1 + N(0,1), seeded with sum(shape);
    cauchy: + 0.2 standard Cauchy; ties: a draw is kept with probability 0.35,
    otherwise it repeats the previous draw of its chain (as an MH chain does)."""
    rng = np.random.default_rng(sum(shape) + seed_shift)
    c, n, p = shape
    x = np.cumsum(rng.standard_normal(shape), axis=1) * 0.1 + rng.standard_normal(shape)
    if kind == "cauchy":
        x = x + 0.2 * rng.standard_cauchy(shape)
    elif kind == "ties":
        keep = rng.random(shape) < 0.35
        keep[:, 0] = True
        src = np.maximum.accumulate(np.where(keep, np.arange(n)[None, :, None], 0), axis=1)
        x = np.take_along_axis(x, src, axis=1)
    elif kind != "ar":
        raise ValueError(kind)
    return np.ascontiguousarray(x.astype(dtype))


def split(x: np.ndarray) -> np.ndarray:
    """[C, N, ...] -> [2C, h, ...]"""
    n = x.shape[1]
    h = n // 2
    return np.concatenate([x[:, :h], x[:, n - h:]], axis=0)


def order_index(m: int, q: float) -> int:
    return int(np.floor((m - 1) * q))


def appb(s: np.ndarray):
    """Appendix B on a split series s[K, h] in f64: (R = sqrt(W/V), ESS, margin),
    margin = the smallest |rho_2i + rho_2i+1| the truncation loop evaluated."""
    s = np.asarray(s, dtype=np.float64)
    k, h = s.shape
    cm = s.mean(axis=1)
    b = ((cm - cm.mean()) ** 2).sum() * h / (k - 1)
    yc = s - cm[:, None]
    w = ((yc * yc).sum(axis=1) / h).mean()
    v = (h - 1) / h * w + b / h
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.sqrt(w / v)
        f = np.fft.rfft(yc, n=2 * h, axis=1)
        acov = np.fft.irfft((f * np.conj(f)).sum(axis=0), n=2 * h)[:h] / h / k
        rho = 1.0 - (w - acov) / v
    mn = rho[0] + rho[1] if h >= 2 else 0.0
    out = 0.0
    margin = np.inf
    for i in range(h // 2):
        pt = rho[2 * i] + rho[2 * i + 1]
        margin = min(margin, abs(pt)) if np.isfinite(pt) else np.nan
        if pt <= 0.0:
            break
        pt = min(pt, mn)
        mn = pt
        out += pt
    with np.errstate(invalid="ignore", divide="ignore"):
        ess = np.float64(k * h) / (-1.0 + 2.0 * out)
    return r, ess, margin


def ranks_of(y: np.ndarray):
    """(r, z) of the pooled values of y[K, h] (ranked in y's dtype)."""
    m = y.size
    r = rankdata(y.reshape(-1), method="average").reshape(y.shape)
    with np.errstate(invalid="ignore"):
        z = ndtri((r - 0.375) / (m + 0.25))
    return r, z


def unsplit(v: np.ndarray, c: int, n: int) -> np.ndarray:
    """[2C, h] -> [C, N] with NaN in an odd N's middle draw."""
    h = n // 2
    out = np.full((c, n), np.nan)
    out[:, :h] = v[:c]
    out[:, n - h:] = v[c:]
    return out


def rank_normalize(x: np.ndarray, folded: bool = False):
    """(ranks, z) as [C, N, P] f64."""
    c, n, p = x.shape
    rk = np.empty(x.shape)
    zz = np.empty(x.shape)
    for j in range(p):
        y = split(x[:, :, j])
        if folded:
            y = np.abs(y.astype(np.float64) - np.median(y.astype(np.float64)))
        r, z = ranks_of(y)
        rk[:, :, j] = unsplit(r, c, n)
        zz[:, :, j] = unsplit(z, c, n)
    return rk, zz


def summary_param(xp: np.ndarray, probs):
    """One parameter xp[C, N]: a dict of its summary and its Geyer margin."""
    y = split(xp)
    m = y.size
    nan = np.nan
    res = dict(mean=nan, sd=nan, quantiles=np.full(len(probs), nan), rhat=nan, ess_bulk=nan, ess_tail=nan,
               margin=np.inf, rhat_bulk=nan, rhat_fold=nan)
    if not np.all(np.isfinite(y)):
        return res
    x64 = xp.astype(np.float64)
    y64 = y.astype(np.float64)
    res["mean"] = x64.mean()
    res["sd"] = x64.std(ddof=1)
    res["quantiles"] = np.quantile(y64.reshape(-1), np.asarray(probs, dtype=np.float64)) if len(probs) else \
        np.empty(0)
    if y.min() == y.max():
        return res
    srt = np.sort(y64.reshape(-1))
    _, z = ranks_of(y)
    _, zf = ranks_of(np.abs(y64 - np.median(y64)))
    rb, eb, m0 = appb(z)
    rf, _, m1 = appb(zf)
    _, e05, m2 = appb((y64 <= srt[order_index(m, 0.05)]).astype(np.float64))
    _, e95, m3 = appb((y64 <= srt[order_index(m, 0.95)]).astype(np.float64))
    res.update(rhat_bulk=1.0 / rb, rhat_fold=1.0 / rf, rhat=np.maximum(1.0 / rb, 1.0 / rf), ess_bulk=eb,
               ess_tail=np.minimum(e05, e95), margin=min(m0, m1, m2, m3) if np.isfinite([m0, m1, m2, m3]).all()
               else nan)
    return res


def summary(x: np.ndarray, probs=(0.05, 0.5, 0.95)) -> dict:
    """The summary of x[C, N, P]: arrays over parameters (quantiles [n_probs, P])."""
    p = x.shape[2]
    rows = [summary_param(x[:, :, j], probs) for j in range(p)]
    out = {k: np.array([r[k] for r in rows]) for k in rows[0] if k != "quantiles"}
    out["quantiles"] = np.stack([r["quantiles"] for r in rows], axis=1) if len(probs) else np.empty((0, p))
    return out
