/* forwarding header: the reference's include path (include/mppi/cost_functions/quadrotor/quadrotor_map_cost.cuh) -> this engine's header.  Paths only. */
#ifndef MPPI_FWD_COST_FUNCTIONS_QUADROTOR_QUADROTOR_MAP_COST_CUH
#define MPPI_FWD_COST_FUNCTIONS_QUADROTOR_QUADROTOR_MAP_COST_CUH
#include "mppi_amd/cost_functions/quadrotor/quadrotor_map_cost.hpp"
#endif
