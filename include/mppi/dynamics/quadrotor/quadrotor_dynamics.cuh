/* forwarding header: the reference's include path (include/mppi/dynamics/quadrotor/quadrotor_dynamics.cuh) -> this engine's header.  Paths only. */
#ifndef MPPI_FWD_DYNAMICS_QUADROTOR_QUADROTOR_DYNAMICS_CUH
#define MPPI_FWD_DYNAMICS_QUADROTOR_QUADROTOR_DYNAMICS_CUH
#include "mppi_amd/dynamics/quadrotor/quadrotor_dynamics.hpp"
#endif
