"""l2hmc_amd -- the L2HMC generalised-leapfrog hot path, MI355X-native.

Python surface = the reference's `utils/dynamics.py`, `utils/sampler.py`, `utils/layers.py`,
`utils/distributions.py` (+ the chain diagnostics of `utils/func_utils.py`, the loss values of `utils/losses.py`,
`utils/notebook_utils.get_hmc_samples`, `utils/ais.py`); compute = the
hand-written HIP kernels of `csrc/` behind the C ABI of `include/l2hmc.h`.
"""
from . import _ffi, diagnostics, distributions, func_utils, layers, losses, multivariate, predictive, quantiles  # noqa: F401
from .dynamics import Dynamics  # noqa: F401
from .sampler import chain_operator, propose, sample_chain, tf_accept  # noqa: F401
from . import tempering  # noqa: F401
from .tempering import ParallelTempering, geometric_ladder  # noqa: F401
from .distributions import LogisticRegression, PoissonRegression, BinomialRegression, NegativeBinomialRegression, ProbitRegression  # noqa: F401
from . import glm  # noqa: F401
from .training import LogisticTrainer  # noqa: F401
from .diagnostics import summarize  # noqa: F401
from .predictive import loo, relative_eff, waic  # noqa: F401
from . import psis  # noqa: F401
from .psis import loo_from_log_lik, relative_eff_from_log_lik  # noqa: F401
from .quantiles import describe  # noqa: F401
from .multivariate import covariance, multi_ess  # noqa: F401
from .warmup import warmup  # noqa: F401  (the function; its module stays importable as `from l2hmc_amd.warmup import ...`)

__all__ = ["Dynamics", "propose", "tf_accept", "chain_operator", "sample_chain", "ParallelTempering", "geometric_ladder",
           "LogisticRegression", "PoissonRegression", "BinomialRegression", "NegativeBinomialRegression", "ProbitRegression", "glm", "LogisticTrainer", "summarize", "diagnostics", "warmup", "predictive", "waic", "loo", "relative_eff", "psis", "loo_from_log_lik", "relative_eff_from_log_lik", "quantiles", "describe",
           "multivariate", "covariance", "multi_ess",
           "layers", "distributions", "func_utils", "losses", "tempering"]
