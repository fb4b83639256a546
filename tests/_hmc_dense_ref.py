"""A numpy float64 transcription of the HMC dense-metric semantics
(include/gmcmc.h gm_hmc_set_dense_adaptation, hmc_dense_device.h): per-chain
dual averaging of the step size and ONE dense metric for all chains,
M^-1 = Sigma = the regularised covariance of the warm-up positions pooled over
every chain, in the window schedule of tests/_hmc_adapt_ref.py. Vectorised
over chains; the momentum normals and accept uniforms come from the caller.
"""
import numpy as np

from tests._hmc_adapt_ref import GAMMA, KAPPA, T0, window_ends


def factor(sigma):
    """A = L^-T (upper triangular) of Sigma = L L^T, or None when Sigma is
    not positive definite."""
    try:
        l = np.linalg.cholesky(sigma)
    except np.linalg.LinAlgError:
        return None
    if not np.all(np.isfinite(l)):
        return None
    return np.linalg.solve(l, np.eye(sigma.shape[0])).T


class Pooled:
    """Float64 pooled statistics with a pivot: c0 = the mean over chains of the
    first accumulated row, s1 = sum (x - c0), S2 = sum (x - c0)(x - c0)^T."""

    def __init__(self, dim):
        self.dim = dim
        self.reset()

    def reset(self):
        self.rn = 0
        self.c0 = np.zeros(self.dim)
        self.s1 = np.zeros(self.dim)
        self.S2 = np.zeros((self.dim, self.dim))

    def add(self, x):
        x = np.asarray(x, dtype=np.float64)
        if self.rn == 0:
            self.c0 = x.mean(axis=0)
        y = x - self.c0
        self.s1 = self.s1 + y.sum(axis=0)
        self.S2 = self.S2 + y.T @ y
        self.rn += 1
        self.C = x.shape[0]

    def covariance(self):
        n = self.rn * self.C
        return (self.S2 - np.outer(self.s1, self.s1) / n) / (n - 1)

    def sigma(self, regularize, jitter):
        s = (1.0 - regularize) * self.covariance() + regularize * np.eye(self.dim)
        i = np.arange(self.dim)
        s[i, i] = np.maximum(s[i, i], max(jitter, 1e-10))
        return s


def run(logp_grad, x0, eps0, L, n_collect, n_discard, adapt, draws, target_accept=0.8, start_buffer=75,
        end_buffer=50, initial_window=25, regularize=0.05, jitter=1e-6, minv0=None, record=False):
    """n_discard warm-up transitions (adapt False: plain burn-in with the
    frozen metric), then n_collect frozen ones. draws(t) -> (z [C, D], u [C]).
    Returns a dict: eps, eps_bar, minv, a, q, samples [C, n_collect, D],
    accepted [T, C], margin (min |log_alpha - ln u| over every decision),
    updates, failed, and with record the positions after every transition."""
    q = np.array(x0, dtype=np.float64)
    C, D = q.shape
    eps = np.broadcast_to(np.asarray(eps0, dtype=np.float64), (C,)).copy()
    eps_bar = eps.copy()
    mu = np.log(10.0 * eps)
    h_bar = np.zeros(C)
    k = 0
    minv = np.eye(D) if minv0 is None else np.array(minv0, dtype=np.float64)
    a = factor(minv)
    stats = Pooled(D)
    ends = set(window_ends(n_discard, start_buffer, end_buffer, initial_window)) if adapt else set()
    lim = n_discard - end_buffer
    updates = failed = 0
    lp, g = logp_grad(q)
    samples = np.empty((C, n_collect, D))
    accepted = np.empty((n_discard + n_collect, C), dtype=bool)
    path = []
    margin = np.inf
    for t in range(n_discard + n_collect):
        z, u = draws(t)
        z = np.asarray(z, dtype=np.float64)
        lnu = np.log(np.asarray(u, dtype=np.float64))
        K0 = 0.5 * np.sum(z * z, axis=1)
        p = z @ a.T  # p = A z
        q1, g1, lp1 = q.copy(), g.copy(), lp.copy()
        e = eps[:, None]
        for _ in range(L):
            p = p + 0.5 * e * g1
            q1 = q1 + e * (p @ minv)  # Sigma symmetric: rows of p times Sigma
            lp1, g1 = logp_grad(q1)
            p = p + 0.5 * e * g1
        K1 = 0.5 * np.sum(p * (p @ minv), axis=1)
        log_alpha = (lp1 - lp) + (K0 - K1)
        acc = log_alpha >= lnu  # NaN rejects
        fin = np.isfinite(lnu) & np.isfinite(log_alpha)
        if fin.any():
            margin = min(margin, float(np.min(np.abs(log_alpha - lnu)[fin])))
        accepted[t] = acc
        q = np.where(acc[:, None], q1, q)
        g = np.where(acc[:, None], g1, g)
        lp = np.where(acc, lp1, lp)
        if record:
            path.append(q.copy())
        with np.errstate(over="ignore", invalid="ignore"):
            alpha = np.minimum(1.0, np.exp(log_alpha))
        alpha = np.where(np.isnan(alpha), 0.0, alpha)
        m = t + 1
        if adapt and m <= n_discard:
            k += 1
            eta = 1.0 / (k + T0)
            h_bar = (1.0 - eta) * h_bar + eta * (target_accept - alpha)
            eps = np.exp(mu - np.sqrt(k) / GAMMA * h_bar)
            eta = k ** (-KAPPA)
            eps_bar = np.exp((1.0 - eta) * np.log(eps_bar) + eta * np.log(eps))
            if start_buffer < m < lim:
                stats.add(q)
                if m in ends and stats.rn >= 5:
                    sig = stats.sigma(regularize, jitter)
                    fa = factor(sig)
                    if fa is None:
                        failed += 1
                    else:
                        minv, a = sig, fa
                        updates += 1
                    stats.reset()
                    eps = eps_bar.copy()
                    mu = np.log(10.0 * eps)
                    h_bar = np.zeros(C)
                    k = 0
            if m == n_discard:
                eps = eps_bar.copy()
        if t >= n_discard:
            samples[:, t - n_discard] = q
    out = dict(eps=eps, eps_bar=eps_bar, minv=minv, a=a, q=q, samples=samples, accepted=accepted, margin=margin,
               updates=updates, failed=failed,
               accept_sampling=float(accepted[n_discard:].mean()) if n_collect else float("nan"))
    if record:
        out["path"] = np.array(path)
    return out
