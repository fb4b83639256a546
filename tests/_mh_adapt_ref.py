"""A numpy float64 transcription of the MH warm-up semantics
(include/gmcmc.h gm_mh_set_adaptation, mh_adapt_device.h): per-chain dual
averaging of the proposal scale and a per-chain diagonal proposal shape from
the Welford variance of the warm-up positions in the shared window schedule.
Vectorised over chains; the proposal normals and accept uniforms come from the
caller, so the GPU tests drive it with the engine's own draws and the CPU
tests with numpy's.
"""
import numpy as np

from tests._hmc_adapt_ref import GAMMA, KAPPA, T0, window_ends  # noqa: F401  (window_ends: re-exported)


def diag_gauss_logp(sigma):
    """logp of N(0, diag(sigma^2)) without the constant."""
    prec = 1.0 / np.asarray(sigma, dtype=np.float64) ** 2

    def f(q):
        return -0.5 * np.sum(q * q * prec, axis=1)
    return f


def run(logp, x0, scale0, n_collect, n_discard, mode, draws, target_accept=0.234, start_buffer=75,
        end_buffer=150, initial_window=25, regularize=0.05, jitter=1e-6, diag0=None):
    """n_discard warm-up transitions (mode 0: plain burn-in), then n_collect
    frozen ones. draws(t) -> (z [C, D], u [C]) for transition t = 0, 1, ...
    Returns a dict: scale, scale_bar, diag, q, samples [C, n_collect, D],
    accepted [T, C], margin (min |log_alpha - ln u| over every decision),
    accept_sampling (mean acceptance of the collected transitions)."""
    q = np.array(x0, dtype=np.float64)
    C, D = q.shape
    scale = np.broadcast_to(np.asarray(scale0, dtype=np.float64), (C,)).copy()
    scale_bar = scale.copy()
    mu = np.log(10.0 * scale)
    h_bar = np.zeros(C)
    k = 0
    diag = np.ones((C, D)) if diag0 is None else np.array(np.broadcast_to(diag0, (C, D)), dtype=np.float64)
    rn, rmean, rm2 = 0, np.zeros((C, D)), np.zeros((C, D))
    ends = set(window_ends(n_discard, start_buffer, end_buffer, initial_window)) if mode == 2 else set()
    lim = n_discard - end_buffer
    lp = logp(q)
    samples = np.empty((C, n_collect, D))
    accepted = np.empty((n_discard + n_collect, C), dtype=bool)
    margin = np.inf
    for t in range(n_discard + n_collect):
        z, u = draws(t)
        z = np.asarray(z, dtype=np.float64)
        with np.errstate(divide="ignore"):
            lnu = np.log(np.asarray(u, dtype=np.float64))
        f = scale[:, None] * diag
        y = q + z * f
        lp1 = logp(y)
        log_alpha = lp1 - lp
        acc = log_alpha > lnu  # strict; NaN rejects
        fin = np.isfinite(lnu) & np.isfinite(log_alpha)
        if fin.any():
            margin = min(margin, float(np.min(np.abs(log_alpha - lnu)[fin])))
        accepted[t] = acc
        q = np.where(acc[:, None], y, q)
        lp = np.where(acc, lp1, lp)
        m = t + 1
        if mode and m <= n_discard:
            with np.errstate(over="ignore", invalid="ignore"):
                alpha = np.minimum(1.0, np.exp(log_alpha))
            alpha = np.where(np.isnan(alpha), 0.0, alpha)
            k += 1
            eta = 1.0 / (k + T0)
            h_bar = (1.0 - eta) * h_bar + eta * (target_accept - alpha)
            scale = np.exp(mu - np.sqrt(k) / GAMMA * h_bar)
            eta = k ** (-KAPPA)
            scale_bar = np.exp((1.0 - eta) * np.log(scale_bar) + eta * np.log(scale))
            if mode == 2 and start_buffer < m < lim:
                rn += 1
                d1 = q - rmean
                rmean = rmean + d1 / rn
                rm2 = rm2 + d1 * (q - rmean)
                if m in ends and rn >= 5:
                    v = np.maximum((1.0 - regularize) * rm2 / (rn - 1) + regularize, max(jitter, 1e-10))
                    diag = np.sqrt(v)
                    rn, rmean, rm2 = 0, np.zeros((C, D)), np.zeros((C, D))
                    scale = scale_bar.copy()
                    mu = np.log(10.0 * scale)
                    h_bar = np.zeros(C)
                    k = 0
            if m == n_discard:
                scale = scale_bar.copy()
        if t >= n_discard:
            samples[:, t - n_discard] = q
    return dict(scale=scale, scale_bar=scale_bar, diag=diag, q=q, samples=samples, accepted=accepted,
                margin=margin, accept_sampling=float(accepted[n_discard:].mean()) if n_collect else float("nan"))


def lag1_autocorr(samples, coord):
    """Lag-1 autocorrelation of one coordinate of samples [C, N, D], pooled
    over chains with each chain's mean removed."""
    x = np.asarray(samples, dtype=np.float64)[:, :, coord]
    x = x - x.mean(axis=1, keepdims=True)
    return float(np.sum(x[:, 1:] * x[:, :-1]) / np.sum(x * x))


# ---- the statistical test's shape and intervals (CPU transcription and GPU alike) ----
# Each interval is followed by the transcription's value over seeds 0..3 and
# both starts (proposal_std 8 and 0.01).
SIGMA = np.geomspace(0.5, 8.0, 8)
N_CHAINS, N_COLLECT, N_DISCARD = 256, 500, 1000


def check_control(accept):
    assert accept < 0.02, accept  # 0.000


def check_mode1(accept, scale, scale_bar, diag, samples):
    assert 0.17 <= accept <= 0.28, accept  # 0.214-0.226
    assert 0.9 <= np.median(scale) <= 1.4, np.median(scale)  # 1.105-1.146
    assert np.all(diag == 1.0)
    np.testing.assert_array_equal(scale, scale_bar)
    r = lag1_autocorr(samples, 7)
    assert r >= 0.975, r  # 0.988-0.989


def check_mode2(accept, scale, scale_bar, diag, samples):
    assert 0.13 <= accept <= 0.26, accept  # 0.178-0.189
    ratio = np.median(np.asarray(diag, dtype=np.float64) / SIGMA, axis=0)
    assert np.all((0.65 <= ratio) & (ratio <= 1.3)), ratio  # 0.82-1.04
    var = np.asarray(samples, dtype=np.float64).reshape(-1, 8).var(axis=0) / SIGMA ** 2
    assert np.all((0.8 <= var) & (var <= 1.2)), var  # 0.94-1.03
    np.testing.assert_array_equal(scale, scale_bar)
    r = lag1_autocorr(samples, 7)
    assert r <= 0.96, r  # 0.931-0.942


def moves(samples):
    """Acceptance of the collected transitions: the share of consecutive rows
    that differ (an accepted proposal moves every coordinate)."""
    return float(np.mean(np.any(samples[:, 1:] != samples[:, :-1], axis=2)))
