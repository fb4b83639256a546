"""general_mcmc_amd — MI355X-native many-chain HMC / NUTS / Metropolis-Hastings.

Drop-in for the hot path of SauersML/general-mcmc (HMC, batched HMC, NUTS,
MH via ChainRunner, split-R-hat/ESS): the same facades and conventions, with
every transition computed by hand-written gfx950 HIP kernels in libgmcmc.so
(include/gmcmc.h is the C ABI). There is no CPU fallback.
"""
from . import _lib, batch_vector
from ._lib import GMError
from .core import init, init_det, init_with_seed
from .distributions import (GLM, CustomTarget, DenseGaussian, DiffableGaussian2D, Gaussian2D,
                            IsotropicGaussian, Rosenbrock2D, RosenbrockND)
from .hmc import HMC, HMCAdaptConfig
from .metropolis_hastings import MetropolisHastings, MHAdaptConfig
from .nuts import NUTS, MassMatrix, NUTSChain, NUTSMassMatrixConfig
from .stats import (BasicStats, ChainStats, GLMLoo, GLMPrediction, MultiChainTracker, Progress, RunStats, SamplerStats,
                    StatsSummary, Summary, basic_stats, rank_normalize, split_rhat_mean_ess, summary)

__all__ = [
    "HMC", "NUTS", "NUTSChain", "MetropolisHastings", "RosenbrockND", "Rosenbrock2D",
    "IsotropicGaussian", "DiffableGaussian2D", "DenseGaussian", "Gaussian2D", "CustomTarget", "GLM", "init",
    "init_det",
    "init_with_seed", "split_rhat_mean_ess", "basic_stats", "BasicStats", "RunStats", "GMError",
    "batch_vector", "MultiChainTracker", "ChainStats", "Progress", "NUTSMassMatrixConfig", "MassMatrix",
    "HMCAdaptConfig", "MHAdaptConfig", "Summary", "summary", "rank_normalize", "SamplerStats", "StatsSummary",
    "GLMPrediction", "GLMLoo",
]
