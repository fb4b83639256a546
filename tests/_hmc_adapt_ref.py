"""A numpy float64 transcription of the HMC warm-up semantics
(include/gmcmc.h gm_hmc_set_adaptation, hmc_adapt_device.h): per-chain dual
averaging of the step size and a per-chain diagonal metric from the Welford
variance of the warm-up positions in the NUTS window schedule. Vectorised over
chains; the momentum normals and accept uniforms come from the caller, so the
GPU tests drive it with the engine's own draws and the CPU tests with numpy's.
"""
import numpy as np

GAMMA, T0, KAPPA = 0.05, 10.0, 0.75


def window_ends(n_discard, start_buffer, end_buffer, initial_window):
    """Transition indices m (1-based) at which a warm-up window ends."""
    lim = n_discard - end_buffer if n_discard > end_buffer else 0
    sched_len = max(initial_window, 10)
    sched_next = max(start_buffer, 1) + sched_len
    ends = []
    for m in range(1, n_discard + 1):
        if m <= start_buffer or not m < lim:
            continue
        if m >= sched_next or m + 1 >= lim:
            sched_next += sched_len
            sched_len = min(2 * sched_len, 400)
            ends.append(m)
    return ends


def diag_gauss(sigma):
    """logp and gradient of N(0, diag(sigma^2)) without the constant."""
    prec = 1.0 / np.asarray(sigma, dtype=np.float64) ** 2

    def f(q):
        return -0.5 * np.sum(q * q * prec, axis=1), -q * prec
    return f


def run(logp_grad, x0, eps0, L, n_collect, n_discard, mode, draws, target_accept=0.8, start_buffer=75,
        end_buffer=50, initial_window=25, regularize=0.05, jitter=1e-6, dinv0=None):
    """n_discard warm-up transitions (mode 0: plain burn-in), then n_collect
    frozen ones. draws(t) -> (z [C, D], u [C]) for transition t = 0, 1, ...
    Returns a dict: eps, eps_bar, dinv, dsq, q, samples [C, n_collect, D],
    accepted [T, C], margin (min |log_alpha - ln u| over every decision),
    accept_sampling (mean acceptance of the collected transitions)."""
    q = np.array(x0, dtype=np.float64)
    C, D = q.shape
    eps = np.broadcast_to(np.asarray(eps0, dtype=np.float64), (C,)).copy()
    eps_bar = eps.copy()
    mu = np.log(10.0 * eps)
    h_bar = np.zeros(C)
    k = 0
    dinv = np.ones((C, D)) if dinv0 is None else np.array(np.broadcast_to(dinv0, (C, D)), dtype=np.float64)
    dsq = 1.0 / np.sqrt(dinv)
    rn, rmean, rm2 = 0, np.zeros((C, D)), np.zeros((C, D))
    ends = set(window_ends(n_discard, start_buffer, end_buffer, initial_window)) if mode == 2 else set()
    lim = n_discard - end_buffer
    lp, g = logp_grad(q)
    samples = np.empty((C, n_collect, D))
    accepted = np.empty((n_discard + n_collect, C), dtype=bool)
    margin = np.inf
    for t in range(n_discard + n_collect):
        z, u = draws(t)
        z = np.asarray(z, dtype=np.float64)
        lnu = np.log(np.asarray(u, dtype=np.float64))
        K0 = 0.5 * np.sum(z * z, axis=1)
        p = dsq * z
        q1, g1, lp1 = q.copy(), g.copy(), lp.copy()
        e = eps[:, None]
        for _ in range(L):
            p = p + 0.5 * e * g1
            q1 = q1 + (e * dinv) * p
            lp1, g1 = logp_grad(q1)
            p = p + 0.5 * e * g1
        K1 = 0.5 * np.sum(dinv * p * p, axis=1)
        log_alpha = (lp1 - lp) + (K0 - K1)
        acc = log_alpha >= lnu  # NaN rejects
        fin = np.isfinite(lnu) & np.isfinite(log_alpha)
        if fin.any():
            margin = min(margin, float(np.min(np.abs(log_alpha - lnu)[fin])))
        accepted[t] = acc
        q = np.where(acc[:, None], q1, q)
        g = np.where(acc[:, None], g1, g)
        lp = np.where(acc, lp1, lp)
        with np.errstate(over="ignore", invalid="ignore"):
            alpha = np.minimum(1.0, np.exp(log_alpha))
        alpha = np.where(np.isnan(alpha), 0.0, alpha)
        m = t + 1
        if mode and m <= n_discard:
            k += 1
            eta = 1.0 / (k + T0)
            h_bar = (1.0 - eta) * h_bar + eta * (target_accept - alpha)
            eps = np.exp(mu - np.sqrt(k) / GAMMA * h_bar)
            eta = k ** (-KAPPA)
            eps_bar = np.exp((1.0 - eta) * np.log(eps_bar) + eta * np.log(eps))
            if mode == 2 and start_buffer < m < lim:
                rn += 1
                d1 = q - rmean
                rmean = rmean + d1 / rn
                rm2 = rm2 + d1 * (q - rmean)
                if m in ends and rn >= 5:
                    v = np.maximum((1.0 - regularize) * rm2 / (rn - 1) + regularize, max(jitter, 1e-10))
                    dinv, dsq = v, 1.0 / np.sqrt(v)
                    rn, rmean, rm2 = 0, np.zeros((C, D)), np.zeros((C, D))
                    eps = eps_bar.copy()
                    mu = np.log(10.0 * eps)
                    h_bar = np.zeros(C)
                    k = 0
            if m == n_discard:
                eps = eps_bar.copy()
        if t >= n_discard:
            samples[:, t - n_discard] = q
    return dict(eps=eps, eps_bar=eps_bar, dinv=dinv, dsq=dsq, q=q, samples=samples, accepted=accepted,
                margin=margin, accept_sampling=float(accepted[n_discard:].mean()) if n_collect else float("nan"))
