"""A numpy float64 transcription of the GLM PSIS-LOO's semantics (include/gmcmc.h
gm_glm_loo), written from the statement and from no library, and the yardstick
that the GPU tests hold the device to.

Per data row, with ll_s (s = 1 .. S) the pointwise log-likelihood as float64:
  1. lw_s = -ll_s - max_s(-ll_s)
  2. M = min(floor(0.2 S), ceil(3 sqrt(S / reff)))
  3. M < 5: k = +inf, nothing is smoothed
  4. the tail is the M largest lw; cutoff = max(lw_(S-M), log(DBL_MIN));
     x_j = exp(tail_j) - exp(cutoff), ascending
  5. x_M <= 0 or x_(floor(M/4 + 0.5)) <= 0: k = +inf, nothing is smoothed
  6. Zhang & Stephens (2009): m = 30 + floor(sqrt M), x* = x_(floor(M/4 + 0.5)),
     theta_j = 1/x_M + (1 - sqrt(m / (j - 0.5))) / (3 x*), kappa(theta) = mean_i
     log1p(-theta x_i), l_j = M (log(-theta_j / kappa_j) - kappa_j - 1), w_j =
     1 / sum_j' exp(l_j' - l_j), theta^ = sum_j theta_j w_j, k = kappa(theta^),
     sigma = -k / theta^, then k <- (k M + 5) / (M + 10)
  7. a finite k: tail value j becomes min(log(q_j + exp(cutoff)), 0), q_j =
     sigma expm1(-k log1p(-p_j)) / k, p_j = (j - 0.5) / M (k = 0: -sigma
     log1p(-p_j))
  8. elpd_loo = logsumexp_s(lw_s + ll_s) - logsumexp_s(lw_s), evaluated as
     (m1 - m2) + log(sum_s exp(lw_s + ll_s - m1) / sum_s exp(lw_s - m2)) with
     m1, m2 the two maxima: one logarithm of the quotient. Each log-sum is of
     the size of log S, rounded to its own grid (2^-49 for 8 <= log S < 16);
     their difference would lie on that grid whatever the size of elpd_loo and
     carry up to a step of it as error, which a row's fuzzed runs show only
     when a rounding happens to flip.
A row with a non-finite ll is NaN in both outputs and counted.

The yardstick. Ops(seed) is the same arithmetic with every ll multiplied by
1 +- 4 * 2^-53, every result of exp / log / log1p / expm1 by 1 +- 2 * 2^-53
(random signs) and every sum taken in reversed order: what an equally good
float64 evaluation may give. Per row, sens = |plain - fuzzed|, maximised over
the seeds; the device may differ from the plain run by
16 sens + 2^-50 max(1, |value|) in that row (ratios()).
"""
import numpy as np

LOG_TINY = float(np.log(np.finfo(np.float64).tiny))
FACTOR = 16.0  # DESIGN.md section 3, "The samplers past one column chunk"
FUZZ_SEEDS = (1, 2, 3)


class Ops:
    """The elementary functions and the sum: plain (seed None) or fuzzed."""

    def __init__(self, seed=None):
        self.rng = None if seed is None else np.random.default_rng(seed)

    def _f(self, v, ulps):
        if self.rng is None:
            return v
        v = np.asarray(v, dtype=np.float64)
        return v * (1.0 + self.rng.choice([-1.0, 1.0], size=v.shape) * (ulps * 2.0 ** -53))

    def ll(self, v):
        return self._f(np.asarray(v, dtype=np.float64), 4.0)

    def exp(self, v):
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            return self._f(np.exp(v), 2.0)

    def log(self, v):
        with np.errstate(divide="ignore", invalid="ignore"):
            return self._f(np.log(v), 2.0)

    def log1p(self, v):
        with np.errstate(divide="ignore", invalid="ignore"):
            return self._f(np.log1p(v), 2.0)

    def expm1(self, v):
        with np.errstate(over="ignore", invalid="ignore"):
            return self._f(np.expm1(v), 2.0)

    def sum(self, v, axis=-1):
        v = np.asarray(v, dtype=np.float64)
        if self.rng is not None:
            v = np.ascontiguousarray(np.flip(v, axis=axis))
        with np.errstate(over="ignore", invalid="ignore"):
            return np.sum(v, axis=axis)


PLAIN = Ops()


def tail_len(S, reff=1.0):
    return int(min(np.floor(0.2 * S), np.ceil(3.0 * np.sqrt(S / reff))))


def k_threshold(S):
    with np.errstate(divide="ignore"):
        return float(min(1.0 - 1.0 / np.log10(float(S)), 0.7))


def gpdfit(x, ops=PLAIN, prior=True):
    """(k, sigma) of ascending x [M], M >= 5, x_M > 0 and x* > 0 (step 6)."""
    M = len(x)
    m = 30 + int(np.floor(np.sqrt(M)))
    j = np.arange(1, m + 1)
    xs = x[int(np.floor(M / 4.0 + 0.5)) - 1]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        theta = 1.0 / x[-1] + (1.0 - np.sqrt(m / (j - 0.5))) / (3.0 * xs)
        kap = ops.sum(ops.log1p(-theta[:, None] * x[None, :]), axis=1) / M
        l = M * ((ops.log(-theta / kap) - kap) - 1.0)
        w = 1.0 / ops.sum(ops.exp(l[None, :] - l[:, None]), axis=1)
        th = float(ops.sum(theta * w))
        k = float(ops.sum(ops.log1p(-th * x))) / M
        sigma = -k / th
        if prior:
            k = (k * M + 5.0) / (M + 10.0)
    return k, sigma


def _max_sum(v, ops):
    """(m, sum exp(v - m)), m the maximum: logsumexp(v) = m + log of the sum."""
    m = np.max(v)
    return m, float(ops.sum(ops.exp(v - m)))


def psis_row(ll, reff=1.0, ops=PLAIN, smooth=True):
    """(elpd_loo, k, raw tail ascending [M]) of one row's ll [S]; smooth=False:
    the raw importance-sampling value (k = +inf)."""
    ll = ops.ll(ll)
    S = len(ll)
    M = tail_len(S, reff)
    if not np.all(np.isfinite(ll)):
        return np.nan, np.nan, np.full(M, np.nan)
    neg = -ll
    lw = neg - np.max(neg)
    order = np.argsort(lw, kind="stable")
    tail = order[S - M:]
    raw = lw[tail].copy()
    k = np.inf
    if M >= 5 and smooth:
        cutoff = max(lw[order[S - M - 1]], LOG_TINY)
        ec = float(ops.exp(cutoff))
        x = ops.exp(raw) - ec
        if x[-1] > 0 and x[int(np.floor(M / 4.0 + 0.5)) - 1] > 0:
            k, sigma = gpdfit(x, ops)
            if np.isfinite(k):
                lp = ops.log1p(-(np.arange(1, M + 1) - 0.5) / M)
                with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                    q = -sigma * lp if k == 0 else sigma * ops.expm1(-k * lp) / k
                    lw = lw.copy()
                    lw[tail] = np.minimum(ops.log(q + ec), 0.0)
    m1, s1 = _max_sum(lw + ll, ops)
    m2, s2 = _max_sum(lw, ops)
    return (m1 - m2) + float(ops.log(s1 / s2)), k, raw


def loo(ll, reff=1.0, ops=PLAIN, smooth=True):
    """ll [S, N] (any float dtype) -> elpd_loo, pareto_k [N], tail [N, M], tail_len, n_nonfinite."""
    ll = np.asarray(ll, dtype=np.float64)
    S, N = ll.shape
    M = tail_len(S, reff)
    e, k, t = np.empty(N), np.empty(N), np.empty((N, M))
    for i in range(N):
        e[i], k[i], t[i] = psis_row(ll[:, i], reff, ops, smooth)
    return {"elpd_loo": e, "pareto_k": k, "tail": t, "tail_len": M,
            "n_nonfinite": int(np.sum(~np.all(np.isfinite(ll), axis=0)))}


def raw_tail(ll, reff=1.0):
    """The M largest of -ll - max(-ll) per column, ascending: [N, M] float64."""
    ll = np.asarray(ll, dtype=np.float64)
    S = ll.shape[0]
    M = tail_len(S, reff)
    neg = -ll
    lw = neg - np.max(neg, axis=0)
    return np.ascontiguousarray(np.sort(lw, axis=0)[S - M:].T)


def sensitivity(ll, reff=1.0, seeds=FUZZ_SEEDS, plain=None):
    """max over seeds of |plain - fuzzed| for elpd_loo and pareto_k, per row."""
    plain = plain or loo(ll, reff)
    s = {n: np.zeros(len(plain[n])) for n in ("elpd_loo", "pareto_k")}
    for seed in seeds:
        f = loo(ll, reff, Ops(seed))
        for n in s:
            with np.errstate(invalid="ignore"):
                d = np.abs(plain[n] - f[n])
            s[n] = np.fmax(s[n], np.where(plain[n] == f[n], 0.0, d))  # (equal infinities: 0)
    return s


def ratios(got, ref, sens):
    """max over the rows of dev / (sens + 2^-50 max(1, |value|) / 16) per output,
    every row against its own sens and value: the device passes at <= 16. NaN
    and infinite reference entries must match exactly."""
    out = {}
    for n in ("elpd_loo", "pareto_k"):
        g, r = np.asarray(got[n], dtype=np.float64), ref[n]
        fin = np.isfinite(r)
        assert np.array_equal(np.isnan(g), np.isnan(r)), f"{n}: NaN pattern differs"
        assert np.array_equal(g[~fin & ~np.isnan(r)], r[~fin & ~np.isnan(r)]), f"{n}: infinities differ"
        d = np.abs(g[fin] - r[fin])
        yard = sens[n][fin] + 2.0 ** -50 * np.maximum(1.0, np.abs(r[fin])) / FACTOR
        out[n] = float(np.max(d / yard)) if d.size else 0.0
    return out
