/**
 * QuadrotorQuadraticCost plugin (reference: include/mppi/cost_functions/quadrotor/quadrotor_quadratic_cost.cuh:10-53,
 * quadrotor_quadratic_cost.cu:70-133 — the DEVICE overloads).
 *
 * Quadratic distance of position, velocity and body rates to s_goal, plus an attitude term on the rotation q_diff that takes
 * the state's quaternion to the goal's (math::QuatSubtract): with use_euler the squared roll / pitch / yaw of q_diff, each with
 * its own coefficient; without it q_coeff times the four components of q_diff — NOT squared, as the reference's device code
 * has it (quadrotor_quadratic_cost.cu:93-99; its host overload squares them).
 *
 * Deliberate fix: the reference ends with `sum * (1 - isnan(sum)) + isnan(sum) * MAX_COST_VALUE` (:126, :132), which is NaN
 * whenever sum is (NaN * 0 = NaN).  A NaN sum returns MAX_COST_VALUE here, which is what that line is there for.
 */
#ifndef MPPI_AMD_QUADROTOR_QUADRATIC_COST_HPP_
#define MPPI_AMD_QUADROTOR_QUADRATIC_COST_HPP_

#include "mppi_amd/plugin/cost.hpp"
#include "mppi_amd/dynamics/quadrotor/quadrotor_dynamics.hpp"

struct QuadrotorQuadraticCostParams : public CostParams<4>
{
  float s_goal[13] = { 0, 0, 0,     // x
                       0, 0, 0,     // v
                       1, 0, 0, 0,  // q
                       0, 0, 0 };   // w
  float x_coeff = 1.0f;
  float v_coeff = 1.0f;
  int use_euler = 1;  ///< the reference's bool, four bytes wide so the block is a flat POD (model_params.h)
  float q_coeff = 1.0f;
  float roll_coeff = 1.0f;
  float pitch_coeff = 1.0f;
  float yaw_coeff = 1.0f;
  float w_coeff = 1.0f;
  float terminal_cost_coeff = 0;

  QuadrotorQuadraticCostParams()
  {
    for (int i = 0; i < 4; i++)
      this->control_cost_coeff[i] = 2.0f;
  }
  float* x_goal()
  {
    return &s_goal[0];
  }
  float* v_goal()
  {
    return &s_goal[3];
  }
  float* q_goal()
  {
    return &s_goal[6];
  }
  float* w_goal()
  {
    return &s_goal[10];
  }
};

class QuadrotorQuadraticCost : public Cost<QuadrotorQuadraticCost, QuadrotorQuadraticCostParams, QuadrotorDynamicsParams>
{
public:
  /** no block barrier in the per-step device methods: may run on the role-separated kernels (plugin/parallel_utils.hpp) */
  static constexpr bool MPPI_BARRIER_FREE_STEP = true;
  /** a pure parameter block on the device: role loops may run it straight off the kernel's argument block (engine/kernarg_view.hpp) */
  static constexpr bool MPPI_KERNARG_VIEWABLE = true;
  static constexpr float MAX_COST_VALUE = 1e16;
  QuadrotorQuadraticCost(hipStream_t stream = nullptr)
  {
    bindToStream(stream);
  }

  /** MAX_COST_VALUE for a NaN (see the note at the top of the file) */
  __host__ __device__ static inline float nanToMaxCost(float cost)
  {
    return (cost != cost) ? MAX_COST_VALUE : cost;
  }

  /**
   * quadrotor_quadratic_cost.cu:70-127 in its order of additions: the attitude angles first (use_euler), then the thirteen
   * per-state terms by index, those of the quaternion being q_coeff * q_diff (or zero with use_euler).
   */
  __device__ inline float computeStateCost(float* s, int timestep = 0, float* theta_c = nullptr, int* crash_status = nullptr)
  {
    const QuadrotorQuadraticCostParams& p = this->params_;
    constexpr int Q0 = E_INDEX(OutputIndex, QUAT_W), W0 = E_INDEX(OutputIndex, ANG_VEL_X);
    float q_diff[4];
    mppi::math::QuatSubtract(s + Q0, p.s_goal + Q0, q_diff);

    float sum = 0.0f;
    if (p.use_euler)
    {
      float r_diff, p_diff, y_diff;
      mppi::math::Quat2EulerNWU(q_diff, r_diff, p_diff, y_diff);
      sum += p.roll_coeff * SQ(r_diff);
      sum += p.pitch_coeff * SQ(p_diff);
      sum += p.yaw_coeff * SQ(y_diff);
    }
#pragma unroll
    for (int i = 0; i < OUTPUT_DIM; i++)
    {
      const float d = s[i] - p.s_goal[i];
      float term;
      if (i >= Q0 && i < W0)
        term = p.use_euler ? 0.0f : p.q_coeff * q_diff[i - Q0];
      else
        term = (d * d) * (i < E_INDEX(OutputIndex, VEL_X) ? p.x_coeff : (i < Q0 ? p.v_coeff : p.w_coeff));
      sum += term;
    }
    return nanToMaxCost(sum);
  }

  /** quadrotor_quadratic_cost.cu:129-133 */
  __device__ inline float terminalCost(float* s, float* theta_c = nullptr)
  {
    return nanToMaxCost(this->params_.terminal_cost_coeff * computeStateCost(s));
  }
};

#endif
