// The kernels of glm.hip for the binomial and the negative-binomial family (glm_family.hpp: one log-likelihood, two means): the
// launches glm.hip's entries dispatch to.  See glm_kernels.hpp.
#include "glm_kernels.hpp"

namespace l2hmc {
L2HMC_GLM_LAUNCHES(, BinomialLogit)
L2HMC_GLM_PREDICT(, BinomialLogit)
L2HMC_GLM_PREDICT(, NegBinomialLog)
}  // namespace l2hmc
