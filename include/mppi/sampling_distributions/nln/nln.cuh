/* forwarding header: the reference's include path (include/mppi/sampling_distributions/nln/nln.cuh) -> this engine's header.  Paths only. */
#ifndef MPPI_FWD_SAMPLING_DISTRIBUTIONS_NLN_NLN_CUH
#define MPPI_FWD_SAMPLING_DISTRIBUTIONS_NLN_NLN_CUH
#include "mppi_amd/sampling_distributions/nln.hpp"
#endif
