"""Random-walk Metropolis-Hastings (metropolis_hastings.rs:90-324) driven like
ChainRunner::run (core.rs:219-229): n_discard + n_collect transitions per
chain, output [chains, n_collect, dim] as float64 (the reference's Trace
conversion, core.rs:39-72, 100-110).

Random-walk MH needs no gradient, but its efficiency hangs on the proposal's
scale. A target that has not been explored needs no hand-tuned one:

    sampler = MetropolisHastings.with_adaptation(target, IsotropicGaussian(1.0), x0).seed(42)
    sample = sampler.run(1000, 500)           # the 500 discarded transitions are the warm-up
    scale, scale_bar = sampler.proposal_scales()   # per chain; sampler.proposal_diag() is the shape

The warm-up adapts, per chain, the proposal scale by dual averaging towards
an acceptance of 0.234 and (adaptation "diagonal") a per-coordinate shape, the
standard deviation of the warm-up positions; both are frozen for sampling. The
proposal of chain c is N(x, (scale[c] * diag[c])^2).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _lib
from ._sampler import Sampler
from .distributions import IsotropicGaussian


@dataclass
class MHAdaptConfig:
    """Warm-up of MH (gm_mh_set_adaptation): adaptation is "none", "scale"
    (per-chain proposal scale) or "diagonal" (scale + per-chain diagonal
    shape). The windows are HMCAdaptConfig's except end_buffer: the variance of
    a short last window of correlated random-walk positions is badly low, so
    the windows stop 150 transitions before the warm-up's end."""
    adaptation: str = "diagonal"
    target_accept: float = 0.234
    start_buffer: int = 75
    end_buffer: int = 150
    initial_window: int = 25
    regularize: float = 0.05
    jitter: float = 1e-6

    @property
    def mode(self) -> int:
        modes = {"none": 0, "scale": 1, "diagonal": 2}
        name = self.adaptation.lower()
        if name not in modes:
            raise ValueError(f"unknown adaptation {self.adaptation!r}: one of \"none\", \"scale\", \"diagonal\"")
        return modes[name]


class MetropolisHastings(Sampler):
    _progress_prefix = "Global"
    _progress_interval = 1.0  # seconds between progress reports

    def __init__(self, target, proposal: IsotropicGaussian, initial_states, dtype=None,
                 chain_offset: int = 0):
        if not isinstance(proposal, IsotropicGaussian):
            raise TypeError("the device MH kernel implements the IsotropicGaussian proposal")
        self.proposal = proposal
        super().__init__(lambda lib: lib.gm_mh_create, target, initial_states,
                         dtype if dtype is not None else np.float64, chain_offset, proposal.std)

    def seed(self, seed: int) -> "MetropolisHastings":
        """metropolis_hastings.rs:189-197."""
        return self._seed(seed)

    set_seed = seed

    @classmethod
    def with_adaptation(cls, target, proposal: IsotropicGaussian, initial_states,
                        cfg: MHAdaptConfig | None = None, **kw) -> "MetropolisHastings":
        """An MH sampler whose next run's discarded transitions are the
        warm-up; proposal.std is every chain's starting scale."""
        s = cls(target, proposal, initial_states, **kw)
        return s.set_adaptation(cfg if cfg is not None else MHAdaptConfig())

    def set_adaptation(self, cfg: MHAdaptConfig) -> "MetropolisHastings":
        """Arm (or re-arm) the warm-up; adaptation "none" drops the per-chain
        scales and shape and returns to the creation proposal."""
        _lib.check(self._lib.gm_mh_set_adaptation(
            self._h, cfg.mode, cfg.target_accept, cfg.start_buffer, cfg.end_buffer, cfg.initial_window,
            cfg.regularize, cfg.jitter))
        return self

    def proposal_scales(self) -> tuple[np.ndarray, np.ndarray]:
        """Per-chain (scale, scale_bar), float64 [n_chains]."""
        sc = np.empty(self.n_chains, dtype=np.float64)
        bar = np.empty(self.n_chains, dtype=np.float64)
        _lib.check(self._lib.gm_mh_get_proposal_scales(self._h, _lib.ptr(sc), _lib.ptr(bar)))
        return sc, bar

    def set_proposal_scales(self, scale) -> "MetropolisHastings":
        sc = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, dtype=np.float64), (self.n_chains,)))
        _lib.check(self._lib.gm_mh_set_proposal_scales(self._h, _lib.ptr(sc)))
        return self

    def proposal_diag(self) -> np.ndarray:
        """The per-chain diagonal proposal shape, [n_chains, dim]."""
        d = np.empty((self.n_chains, self.dim), dtype=self.dtype)
        _lib.check(self._lib.gm_mh_get_proposal_diag(self._h, _lib.ptr(d)))
        return d

    def set_proposal_diag(self, diag) -> "MetropolisHastings":
        """diag per chain: [n_chains, dim], or [dim] for every chain; entries > 0."""
        d = np.ascontiguousarray(np.broadcast_to(np.asarray(diag, dtype=self.dtype), (self.n_chains, self.dim)))
        _lib.check(self._lib.gm_mh_set_proposal_diag(self._h, _lib.ptr(d)))
        return self

    def run(self, n_collect: int, n_discard: int) -> np.ndarray:
        return super().run(n_collect, n_discard).astype(np.float64, copy=False)

    def run_progress(self, n_collect: int, n_discard: int, progress=None, interval=None):
        """ChainRunner::run_progress (core.rs:251-403): f64 samples + RunStats,
        with every chain's ChainTracker stepped on the device each transition."""
        out, stats = super().run_progress(n_collect, n_discard, progress, interval)
        return out.astype(np.float64, copy=False), stats
