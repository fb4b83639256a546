"""The HMC transition of tests/_hmc_adapt_ref.py (identity metric; frozen step
size or its dual averaging), keeping what the sampler statistics record of
every transition: the energy K0 - logp after the momentum refresh, the
acceptance statistic min(1, exp(log_alpha)) (NaN -> 0), the step size the
transition integrated with, the accept decision and the divergence flag
!(log_alpha > -1000). numpy float64; the arithmetic is _hmc_adapt_ref.run's
line for line (tests/test_hmc_stats_ref.py holds the two together)."""
import numpy as np

from tests._hmc_adapt_ref import GAMMA, KAPPA, T0


def run(logp_grad, x0, eps0, L, n_collect, n_discard, mode, draws, target_accept=0.8):
    """mode 0: frozen step sizes; 1: dual averaging during the n_discard
    warm-up transitions. draws(t) -> (z [C, D], u [C]). Returns a dict of
    [T, C] arrays energy, accept_stat, step_size, accepted, divergent, and
    samples [C, n_collect, D], eps, eps_bar, q, margin."""
    q = np.array(x0, dtype=np.float64)
    C, D = q.shape
    T = n_discard + n_collect
    eps = np.broadcast_to(np.asarray(eps0, dtype=np.float64), (C,)).copy()
    eps_bar = eps.copy()
    mu = np.log(10.0 * eps)
    h_bar = np.zeros(C)
    k = 0
    lp, g = logp_grad(q)
    samples = np.empty((C, n_collect, D))
    out = {n: np.empty((T, C)) for n in ("energy", "accept_stat", "step_size")}
    out.update({n: np.empty((T, C), dtype=bool) for n in ("accepted", "divergent")})
    margin = np.inf
    for t in range(T):
        z, u = draws(t)
        z = np.asarray(z, dtype=np.float64)
        lnu = np.log(np.asarray(u, dtype=np.float64))
        K0 = 0.5 * np.sum(z * z, axis=1)
        p = z.copy()
        q1, g1, lp1 = q.copy(), g.copy(), lp.copy()
        e = eps[:, None]
        for _ in range(L):
            p = p + 0.5 * e * g1
            q1 = q1 + e * p
            lp1, g1 = logp_grad(q1)
            p = p + 0.5 * e * g1
        K1 = 0.5 * np.sum(p * p, axis=1)
        log_alpha = (lp1 - lp) + (K0 - K1)
        acc = log_alpha >= lnu  # NaN rejects
        fin = np.isfinite(lnu) & np.isfinite(log_alpha)
        if fin.any():
            margin = min(margin, float(np.min(np.abs(log_alpha - lnu)[fin])))
        with np.errstate(over="ignore", invalid="ignore"):
            alpha = np.minimum(1.0, np.exp(log_alpha))
        alpha = np.where(np.isnan(alpha), 0.0, alpha)
        out["energy"][t] = K0 - lp
        out["accept_stat"][t] = alpha
        out["step_size"][t] = eps
        out["accepted"][t] = acc
        out["divergent"][t] = ~(log_alpha > -1000.0)
        q = np.where(acc[:, None], q1, q)
        g = np.where(acc[:, None], g1, g)
        lp = np.where(acc, lp1, lp)
        m = t + 1
        if mode and m <= n_discard:
            k += 1
            eta = 1.0 / (k + T0)
            h_bar = (1.0 - eta) * h_bar + eta * (target_accept - alpha)
            eps = np.exp(mu - np.sqrt(k) / GAMMA * h_bar)
            eta = k ** (-KAPPA)
            eps_bar = np.exp((1.0 - eta) * np.log(eps_bar) + eta * np.log(eps))
            if m == n_discard:
                eps = eps_bar.copy()
        if t >= n_discard:
            samples[:, t - n_discard] = q
    out.update(samples=samples, eps=eps, eps_bar=eps_bar, q=q, margin=margin)
    return out
