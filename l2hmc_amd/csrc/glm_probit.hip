// The kernels of glm.hip for binomial regression with the probit link (glm_family.hpp, ProbitBinomial): the launches glm.hip's
// entries dispatch to.  See glm_kernels.hpp.
#include "glm_kernels.hpp"

namespace l2hmc {
L2HMC_GLM_LAUNCHES(, ProbitBinomial)
L2HMC_GLM_PREDICT(, ProbitBinomial)
}  // namespace l2hmc
