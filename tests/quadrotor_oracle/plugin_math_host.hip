/**
 * plugin_math_host.hip — the HOST forms of the quaternion helpers the product ships (include/mppi_amd/plugin/math_utils.hpp,
 * __host__ __device__), exported for ctypes.  TEST CODE ONLY.  Compiled by tests/quadrotor_oracle/__init__.py with hipcc for the
 * host alone; tests/test_quadrotor.py holds these to float64 and to the CPU restatement's own copies, which stay a second
 * opinion.  It also fills the two POD parameter blocks of model_params.h from the plugin's parameter classes, so that the layout a
 * C or C++ caller hands to mppi_set_dynamics_params / mppi_set_cost_params is checked against the classes it is copied over.
 */
#include "mppi_amd/plugin/math_utils.hpp"
#include "mppi_amd/cost_functions/quadrotor/quadrotor_quadratic_cost.hpp"
#include "mppi_amd/model_params.h"

#include <cstring>

static_assert(sizeof(mppi_quadrotor_dynamics_params) == sizeof(QuadrotorDynamicsParams), "POD block and plugin parameters differ");
static_assert(sizeof(mppi_quadrotor_cost_params) == sizeof(QuadrotorQuadraticCostParams), "POD block and plugin parameters differ");

extern "C" {
/** which: 0 QuatMultiply(in[0:4], in[4:8]) -> out[4];  1 QuatInv(in[0:4]) -> out[4];  2 QuatSubtract(in[0:4], in[4:8]) -> out[4];
 *  3 Quat2EulerNWU(in[0:4]) -> out[3];  4 Quat2DCM(in[0:4]) -> out[9] row-major;  5 omega2edot(in[0], in[1], in[2], in[3:7]) -> out[4];
 *  6 QuatMultiply(in[0:4], in[4:8], normalize = false) -> out[4];  7 Quat2DCMColumn3(in[0:4]) -> out[3].  Returns the count. */
int plugin_quat_eval(int which, const float* in, float* out)
{
  using namespace mppi::math;
  switch (which)
  {
    case 0: QuatMultiply(in, in + 4, out); return 4;
    case 1: QuatInv(in, out); return 4;
    case 2: QuatSubtract(in, in + 4, out); return 4;
    case 3: Quat2EulerNWU(in, out[0], out[1], out[2]); return 3;
    case 4:
    {
      float M[3][3];
      Quat2DCM(in, M);
      memcpy(out, M, sizeof(M));
      return 9;
    }
    case 5: omega2edot(in[0], in[1], in[2], in + 3, out); return 4;
    case 6: QuatMultiply(in, in + 4, out, false); return 4;
    case 7: Quat2DCMColumn3(in, out); return 3;
  }
  return -1;
}
float plugin_gravity()
{
  return mppi::math::GRAVITY;
}
/** the plugin classes' default parameters, copied out byte for byte as the POD blocks, and the model's default ranges / zero control */
void plugin_default_params(mppi_quadrotor_dynamics_params* dyn, mppi_quadrotor_cost_params* cost)
{
  const QuadrotorDynamicsParams d;
  const QuadrotorQuadraticCostParams c;
  memcpy(dyn, &d, sizeof(d));
  memcpy(cost, &c, sizeof(c));
}
float plugin_nan_to_max_cost(float cost)
{
  return QuadrotorQuadraticCost::nanToMaxCost(cost);
}
}  // extern "C"
