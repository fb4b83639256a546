"""Data-parallel HMC (hmc.rs:75-339 over batched_hmc.rs:29-216).

    sampler = HMC(RosenbrockND(), init_det(4096, 64, np.float32), 0.01, 50).set_seed(42)
    sample = sampler.run(100, 100)            # [chains, n_collect, dim]
    sample, stats = sampler.run_progress(100, 100)

One transition of every chain is one pass of the fused gfx950 kernel
(momentum draw, kinetic energy, L leapfrogs with the analytic gradient,
Metropolis accept); positions stay on the device between calls.

A target that has not been explored needs no hand-tuned step size:

    sampler = HMC.with_adaptation(target, init, 1.0, 10, HMCAdaptConfig()).set_seed(42)
    sample = sampler.run(1000, 400)           # the 400 discarded transitions are the warm-up
    eps, eps_bar = sampler.step_sizes()       # per chain; sampler.metric() is M^-1 and sqrt(M)

The warm-up adapts, per chain, the step size by dual averaging and (mode
"diagonal") a diagonal metric from the positions' variance; both are frozen
for sampling. M^-1 is the regularised sample variance (the Stan / PyMC
convention; the NUTS facade follows the reference and reports 1/var).

A target whose scales are rotated against the axes (a correlated posterior)
needs a dense metric, which no diagonal one replaces:

    cfg = HMCAdaptConfig(adaptation="dense")
    sampler = HMC.with_adaptation(target, init, 0.5, 3, cfg).set_seed(42)
    sample = sampler.run(1000, 400)
    minv, a_factor = sampler.dense_metric()   # Sigma and A = L^-T, float64 [dim, dim]

Mode "dense" keeps the per-chain step sizes and adapts ONE metric for all
chains, M^-1 = the regularised covariance of the warm-up positions pooled over
every chain (thousands of chains estimate it from a short window). It assumes
that all chains target one distribution and are roughly in place by the first
window. 2 <= dim <= 64 at the default layout, built-in targets and user
targets (CustomTarget) alike. On a whitened
target a trajectory of length eps * L near a multiple of pi resonates: choose
L so that eps_bar * L is about pi / 2.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._sampler import Sampler


@dataclass
class HMCAdaptConfig:
    """Warm-up of HMC (gm_hmc_set_adaptation): adaptation is "none",
    "step_size", "diagonal" (step size + per-chain diagonal metric) or "dense"
    (step size + one dense metric pooled over all chains,
    gm_hmc_set_dense_adaptation); the window defaults are
    NUTSMassMatrixConfig's."""
    adaptation: str = "diagonal"
    target_accept: float = 0.8
    start_buffer: int = 75
    end_buffer: int = 50
    initial_window: int = 25
    regularize: float = 0.05
    jitter: float = 1e-6

    @property
    def mode(self) -> int:
        """gm_hmc_set_adaptation's mode; "dense" has none (its own entry
        point, gm_hmc_set_dense_adaptation) and raises ValueError, as an
        unknown name does."""
        modes = {"none": 0, "step_size": 1, "diagonal": 2}
        name = self.adaptation.lower()
        if name == "dense":
            raise ValueError('adaptation "dense" has no gm_hmc_set_adaptation mode: '
                             "HMC.set_adaptation routes it to gm_hmc_set_dense_adaptation")
        if name not in modes:
            raise ValueError(f"unknown adaptation {self.adaptation!r}: one of "
                             '"none", "step_size", "diagonal", "dense"')
        return modes[name]


class HMC(Sampler):
    _progress_prefix = "HMC"
    _progress_interval = 0.5  # seconds between progress reports

    def __init__(self, target, initial_positions, step_size: float, n_leapfrog: int,
                 dtype=None, chain_offset: int = 0):
        self._step_size = float(step_size)
        self._n_leapfrog = int(n_leapfrog)
        super().__init__(lambda lib: lib.gm_hmc_create, target, initial_positions, dtype,
                         chain_offset, self._step_size, self._n_leapfrog)

    def set_seed(self, seed: int) -> "HMC":
        """hmc.rs:143-148 (engine streams are per sampler, not backend-global)."""
        return self._seed(seed)

    @classmethod
    def with_adaptation(cls, target, initial_positions, step_size: float, n_leapfrog: int,
                        cfg: HMCAdaptConfig | None = None, **kw) -> "HMC":
        """An HMC sampler whose next run's discarded transitions are the
        warm-up; step_size is every chain's starting value."""
        s = cls(target, initial_positions, step_size, n_leapfrog, **kw)
        return s.set_adaptation(cfg if cfg is not None else HMCAdaptConfig())

    def set_adaptation(self, cfg: HMCAdaptConfig) -> "HMC":
        """Arm (or re-arm) the warm-up; adaptation "none" drops the per-chain
        step sizes and metric and returns to the creation step size."""
        if cfg.adaptation.lower() == "dense":
            _lib.check(self._lib.gm_hmc_set_dense_adaptation(
                self._h, cfg.target_accept, cfg.start_buffer, cfg.end_buffer, cfg.initial_window,
                cfg.regularize, cfg.jitter))
            return self
        _lib.check(self._lib.gm_hmc_set_adaptation(
            self._h, cfg.mode, cfg.target_accept, cfg.start_buffer, cfg.end_buffer, cfg.initial_window,
            cfg.regularize, cfg.jitter))
        return self

    def step_sizes(self) -> tuple[np.ndarray, np.ndarray]:
        """Per-chain (epsilon, epsilon_bar), float64 [n_chains]."""
        eps = np.empty(self.n_chains, dtype=np.float64)
        bar = np.empty(self.n_chains, dtype=np.float64)
        _lib.check(self._lib.gm_hmc_get_step_sizes(self._h, _lib.ptr(eps), _lib.ptr(bar)))
        return eps, bar

    def set_step_sizes(self, eps) -> "HMC":
        e = np.ascontiguousarray(np.broadcast_to(np.asarray(eps, dtype=np.float64), (self.n_chains,)))
        _lib.check(self._lib.gm_hmc_set_step_sizes(self._h, _lib.ptr(e)))
        return self

    def metric(self) -> tuple[np.ndarray, np.ndarray]:
        """The per-chain diagonal metric as (M^-1, sqrt(M)), [n_chains, dim] each."""
        d = (self.n_chains, self.dim)
        dinv, dsq = np.empty(d, dtype=self.dtype), np.empty(d, dtype=self.dtype)
        _lib.check(self._lib.gm_hmc_get_metric(self._h, _lib.ptr(dinv), _lib.ptr(dsq)))
        return dinv, dsq

    def set_metric(self, diag_inv) -> "HMC":
        """M^-1 per chain: [n_chains, dim], or [dim] for every chain; entries > 0."""
        m = np.ascontiguousarray(np.broadcast_to(np.asarray(diag_inv, dtype=self.dtype),
                                                 (self.n_chains, self.dim)))
        _lib.check(self._lib.gm_hmc_set_metric(self._h, _lib.ptr(m)))
        return self

    def dense_metric(self) -> tuple[np.ndarray, np.ndarray]:
        """The dense metric shared by all chains as (M^-1 = Sigma, A = L^-T with
        Sigma = L L^T), float64 [dim, dim] each."""
        minv = np.empty((self.dim, self.dim), dtype=np.float64)
        a = np.empty((self.dim, self.dim), dtype=np.float64)
        _lib.check(self._lib.gm_hmc_get_dense_metric(self._h, _lib.ptr(minv), _lib.ptr(a), None, None))
        return minv, a

    def set_dense_metric(self, minv) -> "HMC":
        """M^-1 for all chains: [dim, dim], finite, symmetric, positive definite."""
        m = np.ascontiguousarray(np.asarray(minv, dtype=np.float64))
        if m.shape != (self.dim, self.dim):
            raise ValueError(f"minv must be [{self.dim}, {self.dim}]")
        _lib.check(self._lib.gm_hmc_set_dense_metric(self._h, _lib.ptr(m)))
        return self

    def dense_metric_updates(self) -> tuple[int, int]:
        """(metric updates, failed factorisations) of the dense warm-ups so far."""
        upd, failed = C.c_int64(0), C.c_int64(0)
        _lib.check(self._lib.gm_hmc_get_dense_metric(self._h, None, None, C.byref(upd), C.byref(failed)))
        return int(upd.value), int(failed.value)

    def step_size(self) -> float:
        return self._step_size

    def n_leapfrog(self) -> int:
        return self._n_leapfrog
