"""MI355X-native sparse-GP inference core (collapsed / VFE bound) behind the reference's model-class API.

The directory name follows the project naming (``generalised-gaussian-processes_amd``), which is not a
valid Python identifier: import it through the repo-root shim ``ggp_amd`` (``import ggp_amd``).
"""
from ._lib import KERNEL_IDS, SgpLibraryError, SgpStatusError, load_library  # noqa: F401
from .composite import (CO2_LOG_PRIOR_SD, CO2_SGPMC_PRIORS, CompositeBayesianSparseGPR_HMC, CompositeHmcTarget, CompositeKernel,  # noqa: F401
                        CompositeSgpmcTarget, Factor, co2_kernel, co2_sgpmc_kernel)
from .core import CollapsedBound, NotPositiveDefiniteError, SgpTimeoutError, shard_rows  # noqa: F401
from . import datasets, experiment_tools  # noqa: F401
from .exact_nuts import ExactNutsResult, chain_seed, sample_exact_nuts_batch  # noqa: F401
from .exact_predict import ExactMixturePredictive, mixture_quantiles, predict_exact_batch  # noqa: F401
from .gp_shim import (BernoulliLikelihood, ExactMarginalLogLikelihood, GaussianLikelihood, InducingPointKernel, MaternKernel,  # noqa: F401
                      MultivariateNormal, PoissonLikelihood, RBFKernel, RobustMaxLikelihood, ScaleKernel, ZeroMean, settings)
from .hmc import NUTS, SplitMix, Trace, sample_hmc, sample_nuts, sample_nuts_device  # noqa: F401
from .metrics import negative_log_predictive_mixture_density, nlpd, nlpd_marginal, nlpd_mixture, rmse  # noqa: F401
from .ml2 import Ml2Result, fit_ml2, identification_data, lml_surface  # noqa: F401
from .models import (GPR_HMC, BayesianSparseGPR_HMC, BayesianStochasticVariationalGP, SparseGPR, StochasticVariationalGP,  # noqa: F401
                     VariationalHyperDist, all_in_HMC, full_mixture_posterior_predictive, mixture_posterior_predictive)
from .sgpr_batch import SgprBatchResult, elbo_surface, fit_sgpr_batch  # noqa: F401
from .sgpr_nuts import SgprNutsResult, sample_sgpr_nuts_batch  # noqa: F401
from .sgpr_predict import SgprMixturePredictive, predict_sgpr_batch  # noqa: F401
from .sgp_hmc import (CompositeSgpmcModel, SgpmcModel, get_posterior_predictive_uncertainty_intervals, likelihood_moments,  # noqa: F401
                      predict_sgpmc, train_sgp_hmc, train_sgp_hmc_composite)
from .targets import ExactHmcTarget, HmcTarget, JointHmcTarget, SgpmcTarget, SgpmcTargetBase  # noqa: F401


def __getattr__(name):  # lazy: importing the package must work without a GPU (build / symbol checks)
    if name == "HipEngine":
        from .engine import HipEngine
        return HipEngine
    raise AttributeError(name)
