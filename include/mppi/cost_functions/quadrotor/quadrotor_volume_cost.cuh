/* forwarding header: the include path this cost would have in the reference's tree (include/mppi/cost_functions/quadrotor/quadrotor_volume_cost.cuh; the reference has no such cost) -> this engine's header.  Paths only. */
#ifndef MPPI_FWD_COST_FUNCTIONS_QUADROTOR_QUADROTOR_VOLUME_COST_CUH
#define MPPI_FWD_COST_FUNCTIONS_QUADROTOR_QUADROTOR_VOLUME_COST_CUH
#include "mppi_amd/cost_functions/quadrotor/quadrotor_volume_cost.hpp"
#endif
