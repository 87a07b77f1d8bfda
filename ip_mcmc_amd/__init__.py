"""ip_mcmc_amd — MI355X-native many-chain pCN sampler for Bayesian inverse problems.

Drop-in for the pCN hot path of ochsnerd/ip_mcmc (``ip_mcmc/__init__.py``):
the same class names and signatures, plus a leading chain axis, with the
proposal, the forward map G, the potential and the accept/reject fused into
hand-written HIP kernels for gfx950 (libipmc.so, C-ABI in include/ipmc.h).
"""
from .sampler import MCMCSampler
from .proposer import (
    ConstStepStandardRWProposer,
    ConstSteppCNProposer,
    ProposerBase,
    PWLinear,
    VarStepStandardRWProposer,
    VarSteppCNProposer,
)
from .accepter import (
    AccepterBase,
    BoxConstraint,
    ConstrainAccepter,
    CountedAccepter,
    ProbabilisticAccepter,
    StandardRWAccepter,
    pCNAccepter,
)
from .potential import EvolutionPotential, PotentialBase
from .distribution import DistributionBase, GaussianDistribution
from .forward import (
    BurgersOperator,
    LinearOperator,
    Lorenz63Operator,
    Lorenz96Operator,
    ObservationOperator,
    TwoScaleLorenz96Operator,
)
from .rng import PhiloxRNG, PhiloxStream

# the name report/scripts/stuart_examples.py:6 imports (the package's
# ConstSteppCNProposer under its older name)
pCNProposer = ConstSteppCNProposer
from ._lib import IpmcError, UnsupportedOnDevice
from .diagnostics import convergence, moments_convergence, split_rhat
from .covariance import multivariate_rhat, posterior_covariance
from .posterior import (hist_quantiles, histogramdd, marginal_histograms, support, wasserstein_1d,
                        wasserstein_distance, wasserstein_to_point)
from .ranks import pooled_quantiles, rank_convergence, rank_normalize
from .smc import SMCResult, TemperedSMC, next_temperature, systematic_resample, tempering_sums

__all__ = [
    "TemperedSMC",
    "SMCResult",
    "tempering_sums",
    "next_temperature",
    "systematic_resample",
    "rank_convergence",
    "rank_normalize",
    "pooled_quantiles",
    "convergence",
    "split_rhat",
    "moments_convergence",
    "support",
    "marginal_histograms",
    "histogramdd",
    "hist_quantiles",
    "wasserstein_to_point",
    "wasserstein_1d",
    "wasserstein_distance",
    "posterior_covariance",
    "multivariate_rhat",
    "MCMCSampler",
    "ProposerBase",
    "ConstSteppCNProposer",
    "pCNProposer",
    "VarSteppCNProposer",
    "ConstStepStandardRWProposer",
    "VarStepStandardRWProposer",
    "PWLinear",
    "StandardRWAccepter",
    "AccepterBase",
    "BoxConstraint",
    "ConstrainAccepter",
    "CountedAccepter",
    "ProbabilisticAccepter",
    "pCNAccepter",
    "EvolutionPotential",
    "PotentialBase",
    "DistributionBase",
    "GaussianDistribution",
    "BurgersOperator",
    "LinearOperator",
    "Lorenz63Operator",
    "Lorenz96Operator",
    "ObservationOperator",
    "TwoScaleLorenz96Operator",
    "PhiloxRNG",
    "PhiloxStream",
    "IpmcError",
    "UnsupportedOnDevice",
]
