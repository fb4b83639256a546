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
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _lib
from ._sampler import Sampler


@dataclass
class HMCAdaptConfig:
    """Warm-up of HMC (gm_hmc_set_adaptation): adaptation is "none",
    "step_size" or "diagonal" (step size + diagonal metric); the window
    defaults are NUTSMassMatrixConfig's."""
    adaptation: str = "diagonal"
    target_accept: float = 0.8
    start_buffer: int = 75
    end_buffer: int = 50
    initial_window: int = 25
    regularize: float = 0.05
    jitter: float = 1e-6

    @property
    def mode(self) -> int:
        return {"none": 0, "step_size": 1, "diagonal": 2}[self.adaptation.lower()]


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

    def step_size(self) -> float:
        return self._step_size

    def n_leapfrog(self) -> int:
        return self._n_leapfrog
