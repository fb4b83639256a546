"""A numpy float64 reference of the GLM target (include/gmcmc.h gm_glm_desc,
glm_device.h): canonical link, independent Gaussian prior.

    eta_n = sum_j X[n][j] theta_j + offset_n
    logp  = sum_n (y_n eta_n - A(eta_n)) - 0.5 sum_j theta_j^2 / s_j^2
    g_j   = sum_n X[n][j] (y_n - mu(eta_n)) - theta_j / s_j^2

and the first-order forward error scales of that sum in any summation order,
which the GPU tests multiply by 8 (N + D) u.
"""
import numpy as np

FAMILIES = ("bernoulli_logit", "poisson_log")


class GlmRef:
    def __init__(self, X, y, family, prior_sd=1.0, offset=None):
        assert family in FAMILIES
        self.X = np.asarray(X, dtype=np.float64)
        self.N, self.D = self.X.shape
        self.y = np.asarray(y, dtype=np.float64).reshape(self.N)
        self.family = family
        self.sd = np.broadcast_to(np.asarray(prior_sd, dtype=np.float64), (self.D,)).copy()
        self.offset = np.zeros(self.N) if offset is None else np.asarray(offset, dtype=np.float64).reshape(self.N)

    def rounded(self, dtype):
        """The same model with X, y, offset rounded to dtype (what the device holds)."""
        r = lambda a: np.asarray(a, dtype=dtype).astype(np.float64)
        return GlmRef(r(self.X), r(self.y), self.family, self.sd, r(self.offset))

    def eta(self, theta):
        return np.asarray(theta, dtype=np.float64) @ self.X.T + self.offset  # [C, N]

    def link(self, eta):
        """(A, mu) of eta, without overflow for the Bernoulli family."""
        with np.errstate(over="ignore", invalid="ignore"):
            if self.family == "poisson_log":
                mu = np.exp(eta)
                return mu, mu
            em = np.exp(-np.abs(eta))
            A = np.maximum(eta, 0.0) + np.log1p(em)
            mu = np.where(eta >= 0, 1.0, em) / (1.0 + em)
            return A, mu

    def logp_grad(self, theta):
        theta = np.atleast_2d(np.asarray(theta, dtype=np.float64))
        eta = self.eta(theta)
        A, mu = self.link(eta)
        with np.errstate(over="ignore", invalid="ignore"):
            lp = np.sum(self.y * eta - A, axis=1) - 0.5 * np.sum(theta * theta / self.sd ** 2, axis=1)
            g = (self.y - mu) @ self.X - theta / self.sd ** 2
        return lp, g

    def scales(self, theta):
        """S [C], G [C, D]: |delta logp| <= c (N + D) u S and |delta g_j| <= c (N + D) u G_j to
        first order for any summation order (a_n bounds eta_n's own error scale)."""
        theta = np.atleast_2d(np.asarray(theta, dtype=np.float64))
        eta = self.eta(theta)
        A, mu = self.link(eta)
        a = np.abs(theta) @ np.abs(self.X).T + np.abs(self.offset)  # [C, N]
        ay = np.abs(self.y)
        with np.errstate(over="ignore", invalid="ignore"):  # (a Poisson eta past the exp range: infinite scales)
            S = np.sum(np.abs(self.y * eta) + np.abs(A) + (ay + mu) * a, axis=1) + 0.5 * np.sum(
                theta ** 2 / self.sd ** 2, axis=1)
            G = (ay + mu * (1.0 + a)) @ np.abs(self.X) + np.abs(theta) / self.sd ** 2
        return S, G


def unit_roundoff(dtype):
    return float(np.finfo(dtype).eps) / 2


def synth(N, D, family, seed, offset=True, x_scale=None, theta_scale=1.0):
    """A synthetic data set: X ~ N(0, 1/D) (or x_scale), offset ~ 0.3 N(0, 1), y drawn from the
    model at a random theta."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D)) * (1.0 / np.sqrt(D) if x_scale is None else x_scale)
    off = 0.3 * rng.standard_normal(N) if offset else None
    th = theta_scale * rng.standard_normal(D)
    eta = X @ th + (off if offset else 0.0)
    if family == "bernoulli_logit":
        y = (rng.random(N) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    else:
        y = rng.poisson(np.exp(np.clip(eta, -20, 5))).astype(np.float64)
    return X, y, off


def bound(ref, dtype):
    """8 (N + D) u: the factor of the scales in the evaluation bound (tests/test_gpu_glm.py)."""
    return 8.0 * (ref.N + ref.D) * unit_roundoff(dtype)


def perturbed(ref, tol, seed=1):
    """ref.logp_grad with independent errors uniform in +-tol * scales on the log-density and on
    every gradient entry: an evaluation that just meets the bound tol, for a transcription's
    sensitivity to the rounding of the evaluation."""
    prng = np.random.default_rng(seed)

    def f(q):
        lp, g = ref.logp_grad(q)
        S, G = ref.scales(q)
        with np.errstate(invalid="ignore"):  # (a rejected overflow: infinite scales)
            return lp + tol * S * prng.uniform(-1, 1, lp.shape), g + tol * G * prng.uniform(-1, 1, g.shape)
    return f


# ---- the NUTS cases of tests/test_nuts_ref.py (CPU) and tests/test_gpu_glm.py (GPU) ----
# (N, D, layout or None for the default): two and four column chunks at two row
# passes, and three chunks with the second coordinate slot real
NUTS_SHAPES = [(300, 33, None), (300, 128, None), (70, 65, (64, 2))]
NUTS_RUN = dict(n_chains=4, n_collect=4, n_discard=6, seed=17, max_depth=6, target_accept=0.8)
_nuts_cache = {}


def nuts_case(N, D, family):
    """(reference, gm.GLM arguments, x0 [4, D])."""
    X, y, off = synth(N, D, family, 3)
    x0 = 0.3 * np.random.default_rng(5).standard_normal((NUTS_RUN["n_chains"], D))
    return GlmRef(X, y, family, 2.0, off), dict(X=X, y=y, family=family, prior_sd=2.0, offset=off), x0


def nuts_reference(oracle, N, D, family):
    """The float64 NUTS transcription (tests/_nuts_ref.py) of the case, a second run of it under
    perturbed() at the float64 evaluation bound, and their deviation: (r, r2, sens), stacked
    over chains. Computed once per case."""
    from tests import _nuts_ref
    key = (N, D, family)
    if key not in _nuts_cache:
        ref, _, x0 = nuts_case(N, D, family)
        c = NUTS_RUN
        args = (x0, -1.0, c["n_collect"], c["n_discard"], c["seed"], c["max_depth"], c["target_accept"])
        r = _nuts_ref.stack(_nuts_ref.run(oracle, ref.logp_grad, *args))
        r2 = _nuts_ref.stack(_nuts_ref.run(oracle, perturbed(ref, bound(ref, np.float64)), *args))
        _nuts_cache[key] = (r, r2, _nuts_ref.deviation(r, r2))
    return _nuts_cache[key]
