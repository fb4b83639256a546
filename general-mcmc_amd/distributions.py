"""Built-in targets and the isotropic-Gaussian proposal.

Mirrors the reference's distributions module (distributions.rs): the same
names and parameters, but each target is a descriptor of a device-side
log-density with an analytic gradient (no autodiff graph, hmc.rs:42-61).

    RosenbrockND          distributions.rs:535-555   (a=1, b=100, any dim)
    Rosenbrock2D(a, b)    distributions.rs:495-530
    IsotropicGaussian(s)  distributions.rs:349-406   (target and MH proposal)
    DiffableGaussian2D    distributions.rs:215-320
    DenseGaussian         DiffableGaussian2D generalised to dim D
    Gaussian2D            distributions.rs:161-208   (Target, no norm const)
    CustomTarget          a user target (the Target / GradientTarget traits,
                          distributions.rs:67-110) as HIP source, compiled at
                          run time into the sampler kernels
    GLM                   Bayesian logistic / Poisson regression on a data set
                          (no counterpart in the reference)
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib


class _TargetBase:
    """A device-evaluated target. `dim` is None when the target adapts to the
    sampler's dimension (RosenbrockND, IsotropicGaussian)."""

    dim: int | None = None

    def _fill(self, t: _lib.gm_target, dim: int) -> list:
        raise NotImplementedError

    def to_struct(self, dim: int):
        if self.dim is not None and self.dim != dim:
            # the reference panics here (distributions.rs:267, 302)
            raise ValueError(f"{type(self).__name__}: expected dimension={self.dim}, got {dim}")
        t = _lib.gm_target()
        t.dim = dim
        keep = self._fill(t, dim)
        return t, keep

    # BatchedGradientTarget::unnorm_logp_batch (distributions.rs:67-78), plus the
    # gradient the reference gets from autodiff (hmc.rs:42-61).
    def unnorm_logp_and_grad_batch(self, positions, dtype=None):
        x = np.asarray(positions)
        if dtype is None:
            dtype = x.dtype if x.dtype in (np.float32, np.float64) else np.float64
        x = np.ascontiguousarray(x, dtype=dtype)
        if x.ndim == 1:
            x = x[None, :]
        n, dim = x.shape
        t, keep = self.to_struct(dim)
        lp = np.empty(n, dtype=dtype)
        g = np.empty((n, dim), dtype=dtype)
        lib = _lib.require_gpu()
        _lib.check(lib.gm_target_logp_grad(C.byref(t), _lib.dtype_code(dtype), n, _lib.ptr(x),
                                           _lib.ptr(lp), _lib.ptr(g)))
        del keep
        return lp, g

    def unnorm_logp_batch(self, positions, dtype=None):
        return self.unnorm_logp_and_grad_batch(positions, dtype)[0]

    # GradientTarget::unnorm_logp / unnorm_logp_and_grad (distributions.rs:80-90)
    def unnorm_logp_and_grad(self, position, dtype=None):
        lp, g = self.unnorm_logp_and_grad_batch(np.asarray(position)[None, :], dtype)
        return lp[0], g[0]

    # Target::unnorm_logp (distributions.rs:107-110)
    def unnorm_logp(self, position, dtype=None):
        return self.unnorm_logp_and_grad(position, dtype)[0]


class RosenbrockND(_TargetBase):
    """-sum_{i<D-1} [100 (x_{i+1} - x_i^2)^2 + (1 - x_i)^2]."""

    a = 1.0
    b = 100.0

    def _fill(self, t, dim):
        t.kind = _lib.GM_TARGET_ROSENBROCK
        t.a, t.b = 1.0, 100.0
        return []


class Rosenbrock2D(_TargetBase):
    def __init__(self, a: float = 1.0, b: float = 100.0):
        self.a = float(a)
        self.b = float(b)
        self.dim = 2

    def _fill(self, t, dim):
        t.kind = _lib.GM_TARGET_ROSENBROCK
        t.a, t.b = self.a, self.b
        return []


class IsotropicGaussian(_TargetBase):
    """Zero-mean isotropic Gaussian N(0, std^2 I): a target (any dim) and the
    random-walk proposal of Metropolis-Hastings (x' = x + std * N(0, I))."""

    def __init__(self, std: float = 1.0):
        self.std = float(std)

    def _fill(self, t, dim):
        t.kind = _lib.GM_TARGET_ISO_GAUSS
        t.std = self.std
        return []

    # Proposal::logp (distributions.rs:378-390), including the reference's
    # constant -d/2 ln(var * pi * std^2); host-side helper for tests/diagnostics.
    def proposal_logp(self, frm, to) -> float:
        frm = np.asarray(frm, dtype=np.float64)
        to = np.asarray(to, dtype=np.float64)
        var = self.std * self.std
        lp = float(np.sum(-((to - frm) ** 2) / (2 * var)))
        return lp + -len(frm) * 0.5 * math.log(var * math.pi * self.std * self.std)


class _GaussBase(_TargetBase):
    def __init__(self, mean, cov, norm_const: float | None):
        self.mean = np.ascontiguousarray(np.asarray(mean, dtype=np.float64))
        self.cov = np.ascontiguousarray(np.asarray(cov, dtype=np.float64))
        d = self.mean.shape[0]
        if self.cov.shape != (d, d):
            raise ValueError("cov must be [dim, dim]")
        self.dim = d
        self.inv_cov = np.empty((d, d), dtype=np.float64)
        nc = C.c_double(0.0)
        lib = _lib.load()
        _lib.check(lib.gm_gauss_from_cov(d, _lib.ptr(self.cov), _lib.ptr(self.inv_cov), C.byref(nc)))
        self.log_norm_const = nc.value
        self.norm_const = nc.value if norm_const is None else norm_const

    def _fill(self, t, dim):
        t.kind = _lib.GM_TARGET_GAUSS
        t.mean = self.mean.ctypes.data_as(C.POINTER(C.c_double))
        t.prec = self.inv_cov.ctypes.data_as(C.POINTER(C.c_double))
        t.norm_const = self.norm_const
        return [self.mean, self.inv_cov]


class DiffableGaussian2D(_GaussBase):
    """distributions.rs:215-320: logp includes -(2 ln 2pi + ln|Sigma|)/2."""

    def __init__(self, mean, cov):
        super().__init__(mean, cov, None)
        if self.dim != 2:
            raise ValueError("Gaussian2D: expected dimension=2.")


class DenseGaussian(_GaussBase):
    """Full-covariance Gaussian in D dims (config 3's target)."""

    def __init__(self, mean, cov):
        super().__init__(mean, cov, None)


class Gaussian2D(_GaussBase):
    """distributions.rs:161-208. As a Target: -0.5 d^T Sigma^-1 d (no constant);
    `logp` (Normalized) adds -ln(2 pi) - 0.5 ln|det Sigma|."""

    def __init__(self, mean, cov):
        super().__init__(mean, cov, 0.0)
        if self.dim != 2:
            raise ValueError("Gaussian2D: expected dimension=2.")

    def logp(self, position) -> float:
        c = self.cov
        det = c[0, 0] * c[1, 1] - c[0, 1] * c[1, 0]
        return float(self.unnorm_logp(np.asarray(position, dtype=np.float64))) + (
            -math.log(2.0 * math.pi) - 0.5 * math.log(abs(det)))


class CustomTarget(_TargetBase):
    """A user-defined target, the counterpart of implementing the reference's
    GradientTarget / BatchedGradientTarget traits (distributions.rs:67-110).

    `source` is HIP C++ defining, for T = float and double,

        template <class T>
        __device__ T gm_logp_grad(const T* x, T* g, const T* params);

    which receives one chain's position x[GM_DIM] (GM_DIM is a macro equal to
    `dim`), writes the gradient of the unnormalised log-density to g[GM_DIM]
    and returns the log-density. `params` are copied to the device in the
    sampler's dtype. The source is compiled at run time (hiprtc) together
    with the engine's own HMC / MH / NUTS kernels, one chain per lane
    (layout 1 x dim, dim <= 256); a compile error raises at sampler creation
    with the compiler log. The gradient is the user's: there is no autodiff
    on the device."""

    def __init__(self, source: str, dim: int, params=()):
        self.source = str(source)
        self.dim = int(dim)
        self.params = np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(-1))

    def _fill(self, t, dim):
        t.kind = _lib.GM_TARGET_CUSTOM
        src = self.source.encode()
        t.source = src
        t.params = self.params.ctypes.data_as(C.POINTER(C.c_double))
        t.n_params = self.params.size
        return [src, self.params]

    _KINDS = {"logp": 0, "hmc": 1, "mh": 2, "nuts": 3, "hmc_adapt": 4, "hmc_dense": 5, "mh_adapt": 6}

    def check(self, sampler: str = "hmc", dtype=np.float64) -> None:
        """Compile the source into `sampler`'s kernel ("hmc", "mh", "nuts",
        "hmc_adapt": HMC with per-chain step sizes / metric / warm-up,
        "hmc_dense": HMC with the dense metric, 2 <= dim <= 64, "mh_adapt": MH
        with per-chain proposal scales / shape / warm-up, or "logp")
        without running it; raises GMError with the compiler log."""
        lib = _lib.load()
        _lib.check(lib.gm_custom_target_check(self.source.encode(), _lib.dtype_code(dtype), self.dim,
                                              self._KINDS[sampler]))


class GLM(_TargetBase):
    """Generalised linear model with canonical link and an independent Gaussian
    prior; the chain's position is the coefficient vector theta [D]:

        eta_n = sum_j X[n][j] theta_j + offset_n
        logp  = sum_n (y_n eta_n - A(eta_n)) - 0.5 sum_j theta_j^2 / prior_sd_j^2

    family "bernoulli_logit" (0 <= y <= 1; A = log(1 + exp(eta))) or
    "poisson_log" (y >= 0; A = exp(eta); `offset` is the log exposure).
    The intercept is a column of ones in X. Runs with HMC (and its warm-up)
    and NUTS (identity or diagonal adaptive metric); 1 <= D <= 128."""

    FAMILIES = {"bernoulli_logit": _lib.GM_GLM_BERNOULLI_LOGIT, "poisson_log": _lib.GM_GLM_POISSON_LOG}

    def __init__(self, X, y, family: str = "bernoulli_logit", prior_sd=1.0, offset=None):
        if family not in self.FAMILIES:
            raise ValueError(f"GLM target: family must be one of {sorted(self.FAMILIES)}, got {family!r}")
        X = np.ascontiguousarray(np.asarray(X, dtype=np.float64))
        if X.ndim != 2:
            raise ValueError("GLM target: X must be [n_rows, dim]")
        n, d = X.shape
        if n < 1:
            raise ValueError("GLM target: n_rows must be >= 1")
        if not 1 <= d <= 128:
            raise ValueError("GLM target: dim must be in [1, 128]")
        y = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(-1))
        if y.shape != (n,):
            raise ValueError(f"GLM target: y must be [n_rows] = [{n}], got {list(y.shape)}")
        sd = np.asarray(prior_sd, dtype=np.float64)
        if sd.ndim == 0:
            sd = np.full(d, float(sd))
        sd = np.ascontiguousarray(sd.reshape(-1))
        if sd.shape != (d,):
            raise ValueError(f"GLM target: prior_sd must be a scalar or [dim] = [{d}], got {list(sd.shape)}")
        if offset is not None:
            offset = np.ascontiguousarray(np.asarray(offset, dtype=np.float64).reshape(-1))
            if offset.shape != (n,):
                raise ValueError(f"GLM target: offset must be [n_rows] = [{n}], got {list(offset.shape)}")

        def first(bad):  # index of the first True of a mask
            return int(np.argmax(bad))

        # the C side's checks, in its order and wording
        bad = ~np.isfinite(sd)
        if bad.any():
            raise ValueError(f"GLM target: prior_sd is not finite at column {first(bad)}")
        bad = ~(sd > 0)
        if bad.any():
            raise ValueError(f"GLM target: prior_sd must be > 0 at column {first(bad)}")
        # rows: the first offending row; within it x, then y, its range, the offset
        xb = ~np.isfinite(X)
        yb = ~np.isfinite(y)
        if family == "bernoulli_logit":
            rb, rmsg = ~((y >= 0) & (y <= 1)) & ~yb, "GLM target: bernoulli_logit needs 0 <= y <= 1 at row {}"
        else:
            rb, rmsg = ~(y >= 0) & ~yb, "GLM target: poisson_log needs y >= 0 at row {}"
        ob = ~np.isfinite(offset) if offset is not None else np.zeros(n, dtype=bool)
        found = []
        for rank, (mask, fmt) in enumerate(((xb.any(axis=1), None), (yb, "GLM target: y is not finite at row {}"),
                                            (rb, rmsg), (ob, "GLM target: offset is not finite at row {}"))):
            if mask.any():
                r = first(mask)
                found.append((r, rank, fmt.format(r) if fmt else
                              f"GLM target: x is not finite at row {r}, column {first(xb[r])}"))
        if found:
            raise ValueError(min(found)[2])
        self.X, self.y, self.prior_sd, self.offset = X, y, sd, offset
        self.family = family
        self.n_rows = n
        self.dim = d

    def _fill(self, t, dim):
        dp = C.POINTER(C.c_double)
        desc = _lib.gm_glm_desc()
        desc.family = self.FAMILIES[self.family]
        desc.n_rows = self.n_rows
        desc.x = self.X.ctypes.data_as(dp)
        desc.y = self.y.ctypes.data_as(dp)
        desc.offset = self.offset.ctypes.data_as(dp) if self.offset is not None else None
        desc.prior_sd = self.prior_sd.ctypes.data_as(dp)
        t.kind = _lib.GM_TARGET_GLM
        t.glm = C.pointer(desc)
        return [desc, self.X, self.y, self.offset, self.prior_sd]

    def predict(self, draws, X=None, y=None, offset=None, pointwise: bool = False):
        """Posterior prediction over stored draws, computed on the GPU in the
        draws' dtype and reduced over all of them in f64 (stats.GLMPrediction):
        per data row the mean and sd of eta and of mu and, with y, the lppd and
        the mean and variance of the pointwise log-likelihood (waic()).

        draws: the DeviceSamples of a run on this model (used where they lie,
        n_collect * n_chains draws in stored order) or a host array [..., dim]
        (f32 and f64 are kept, anything else becomes f64).
        X = None: the training rows with their y and offset. With a new X, y
        and offset default to None; without y only eta and mu are returned.
        pointwise: also the matrix ll [n_draws, n_rows] in the draws' dtype
        (at most 2^31 bytes: pass the rows in blocks beyond that)."""
        from ._sampler import DeviceSamples
        from .stats import GLMPrediction
        if X is None:
            if y is not None or offset is not None:
                raise ValueError("GLM predict: y and offset go with a new X")
            X, y, offset = self.X, self.y, self.offset
        else:
            X = np.ascontiguousarray(np.asarray(X, dtype=np.float64))
            if X.ndim != 2 or X.shape[1] != self.dim:
                raise ValueError(f"GLM predict: X must be [n_rows, dim] with dim = {self.dim}")
            n = X.shape[0]
            if y is not None:
                y = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(-1))
                if y.shape != (n,):
                    raise ValueError(f"GLM predict: y must be [n_rows] = [{n}], got {list(y.shape)}")
            if offset is not None:
                offset = np.ascontiguousarray(np.asarray(offset, dtype=np.float64).reshape(-1))
                if offset.shape != (n,):
                    raise ValueError(f"GLM predict: offset must be [n_rows] = [{n}], got {list(offset.shape)}")
        m = X.shape[0]
        if pointwise and y is None:
            raise ValueError("GLM predict: the pointwise log-likelihood needs y")
        dp = C.POINTER(C.c_double)
        desc = _lib.gm_glm_desc()
        desc.family = self.FAMILIES[self.family]
        desc.n_rows = m
        desc.x = X.ctypes.data_as(dp)
        desc.y = y.ctypes.data_as(dp) if y is not None else None
        desc.offset = offset.ctypes.data_as(dp) if offset is not None else None
        desc.prior_sd = None

        if isinstance(draws, DeviceSamples):
            draws._check_live()
            if draws.dim != self.dim:
                raise ValueError(f"GLM predict: the samples have dim {draws.dim}, the model {self.dim}")
            dtype = np.dtype(draws.dtype)
            s = draws.n_collect * draws.n_chains
            host = None
        else:
            host = np.asarray(draws)
            if host.dtype not in (np.float32, np.float64):
                host = host.astype(np.float64)
            if host.ndim < 1 or host.shape[-1] != self.dim:
                raise ValueError(f"GLM predict: draws must be [..., dim] with dim = {self.dim}")
            dtype = host.dtype
            s = int(np.prod(host.shape[:-1], dtype=np.int64))
        if s < 1:
            raise ValueError("GLM predict: no draws")
        # before anything of that size is allocated
        if pointwise and s * m * dtype.itemsize > 2 ** 31:
            raise ValueError(f"GLM predict: the pointwise matrix ({s} x {m} x {dtype.itemsize} bytes) is larger than "
                             "2^31 bytes: pass the rows in blocks")
        if host is not None:
            host = np.ascontiguousarray(host.reshape(s, self.dim))
        names = ["eta_mean", "eta_sd", "mu_mean", "mu_sd"] + (["lppd", "ll_mean", "ll_var"] if y is not None else [])
        f = {k: np.empty(m) for k in names}
        pw = np.empty((s, m), dtype=dtype) if pointwise else None
        out = _lib.gm_glm_predict_out(**{k: a.ctypes.data for k, a in f.items()})
        out.pointwise = pw.ctypes.data if pw is not None else None
        lib = _lib.require_gpu()
        if host is None:
            draws.owner.synchronize()  # an asynchronous run may still be writing them
            _lib.check(lib.gm_glm_predict_device(C.byref(desc), self.dim, _lib.dtype_code(dtype), C.c_void_p(draws.ptr),
                                                 s, self.dim, C.byref(out)))
        else:
            _lib.check(lib.gm_glm_predict(C.byref(desc), self.dim, _lib.dtype_code(dtype), _lib.ptr(host), s,
                                          C.byref(out)))
        return GLMPrediction(f["eta_mean"], f["eta_sd"], f["mu_mean"], f["mu_sd"], f.get("lppd"), f.get("ll_mean"),
                             f.get("ll_var"), pw, s)

    def loo(self, draws, reff: float = 1.0, tail: bool = False, workspace_bytes: int = 0):
        """PSIS-LOO over stored draws, computed on the GPU (stats.GLMLoo): per
        training row the Pareto-smoothed leave-one-out elpd and the Pareto
        shape k of its importance ratios, from the pointwise log-likelihood of
        predict() (same bits); the lppd beside them is predict()'s.

        draws: as for predict(), at most 2^24 of them.
        reff: the relative efficiency of the draws, a positive scalar; the tail
        has min(floor(0.2 S), ceil(3 sqrt(S / reff))) values.
        tail: also the sorted raw tail [n_rows, tail_len], f64, ascending.
        workspace_bytes: the bound of the device workspace (0: the default,
        stats.loo_plan()); the result does not depend on it."""
        from ._sampler import DeviceSamples
        from .stats import GLMLoo, loo_plan
        reff = float(reff)
        if not (np.isfinite(reff) and reff > 0):
            raise ValueError("GLM loo: reff must be finite and > 0")
        n = self.n_rows
        if isinstance(draws, DeviceSamples):
            draws._check_live()
            if draws.dim != self.dim:
                raise ValueError(f"GLM loo: the samples have dim {draws.dim}, the model {self.dim}")
            dtype, host = np.dtype(draws.dtype), None
            s = draws.n_collect * draws.n_chains
        else:
            host = np.asarray(draws)
            if host.dtype not in (np.float32, np.float64):
                host = host.astype(np.float64)
            if host.ndim < 1 or host.shape[-1] != self.dim:
                raise ValueError(f"GLM loo: draws must be [..., dim] with dim = {self.dim}")
            dtype = host.dtype
            s = int(np.prod(host.shape[:-1], dtype=np.int64))
            host = np.ascontiguousarray(host.reshape(s, self.dim))
        if s < 1:
            raise ValueError("GLM loo: no draws")
        # every refusal comes before any device work: the plan refuses what the call would
        m = loo_plan(dtype, s, n, reff, workspace_bytes)["tail_len"]
        pred = self.predict(draws if host is None else host)  # lppd
        elpd, k = np.empty(n), np.empty(n)
        tl = np.empty((n, m)) if tail else None
        out = _lib.gm_glm_loo_out(elpd_loo=elpd.ctypes.data, pareto_k=k.ctypes.data,
                                  tail=tl.ctypes.data if tail else None)
        dp = C.POINTER(C.c_double)
        desc = _lib.gm_glm_desc()
        desc.family = self.FAMILIES[self.family]
        desc.n_rows = n
        desc.x = self.X.ctypes.data_as(dp)
        desc.y = self.y.ctypes.data_as(dp)
        desc.offset = self.offset.ctypes.data_as(dp) if self.offset is not None else None
        desc.prior_sd = None
        lib = _lib.require_gpu()
        if host is None:
            _lib.check(lib.gm_glm_loo_device(C.byref(desc), self.dim, _lib.dtype_code(dtype), C.c_void_p(draws.ptr), s,
                                             self.dim, reff, int(workspace_bytes), C.byref(out)))
        else:
            _lib.check(lib.gm_glm_loo(C.byref(desc), self.dim, _lib.dtype_code(dtype), _lib.ptr(host), s, reff,
                                      int(workspace_bytes), C.byref(out)))
        return GLMLoo(elpd, k, pred.lppd, tl, int(out.tail_len), int(out.n_nonfinite), s)
