/**
 * QuadrotorDynamics plugin (reference: include/mppi/dynamics/quadrotor/quadrotor_dynamics.cuh:10-123,
 * quadrotor_dynamics.cu:4-19 the constructors, :127-188 the device computeDynamics / updateState, :212-234 getZeroState).
 *
 * State (13): position, velocity, attitude quaternion (w, x, y, z), body rates — NWU frame.  Control (4): the three body-rate
 * commands, tracked as first-order lags with time constants tau_*, and the thrust along the body z axis.  After every Euler
 * step the quaternion is scaled back to unit length with a non-negative w.
 *
 * The quaternion helpers are those of plugin/math_utils.hpp (one arithmetic flavour for device and host, see there).
 */
#ifndef MPPI_AMD_QUADROTOR_DYNAMICS_HPP_
#define MPPI_AMD_QUADROTOR_DYNAMICS_HPP_

#include <array>

#include "mppi_amd/plugin/dynamics.hpp"

struct QuadrotorDynamicsParams : public DynamicsParams
{
  enum class StateIndex : int
  {
    POS_X = 0,
    POS_Y,
    POS_Z,
    VEL_X,
    VEL_Y,
    VEL_Z,
    QUAT_W,
    QUAT_X,
    QUAT_Y,
    QUAT_Z,
    ANG_VEL_X,
    ANG_VEL_Y,
    ANG_VEL_Z,
    NUM_STATES
  };
  enum class ControlIndex : int
  {
    ANG_RATE_X = 0,
    ANG_RATE_Y,
    ANG_RATE_Z,
    THRUST,
    NUM_CONTROLS
  };
  enum class OutputIndex : int
  {
    POS_X = 0,
    POS_Y,
    POS_Z,
    VEL_X,
    VEL_Y,
    VEL_Z,
    QUAT_W,
    QUAT_X,
    QUAT_Y,
    QUAT_Z,
    ANG_VEL_X,
    ANG_VEL_Y,
    ANG_VEL_Z,
    NUM_OUTPUTS
  };
  float tau_roll = 0.25f;
  float tau_pitch = 0.25f;
  float tau_yaw = 0.25f;
  float mass = 1.0f;  // kg

  QuadrotorDynamicsParams() = default;
  QuadrotorDynamicsParams(float mass_in) : mass(mass_in){};
};

using namespace MPPI_internal;

class QuadrotorDynamics : public Dynamics<QuadrotorDynamics, QuadrotorDynamicsParams>
{
public:
  /** no block barrier in the per-step device methods: may run on the role-separated kernels (plugin/parallel_utils.hpp) */
  static constexpr bool MPPI_BARRIER_FREE_STEP = true;
  using PARENT_CLASS = Dynamics<QuadrotorDynamics, QuadrotorDynamicsParams>;

  /** thrust in [0, 36] N, hover thrust as the zero control (quadrotor_dynamics.cu:11-19) */
  QuadrotorDynamics(hipStream_t stream = 0) : PARENT_CLASS(stream)
  {
    this->control_rngs_[C_INDEX(THRUST)] = make_float2(0.0f, 36.0f);
    this->zero_control_[C_INDEX(THRUST)] = mppi::math::GRAVITY;
  }
  /** the caller's ranges for all four controls (quadrotor_dynamics.cu:4-9) */
  QuadrotorDynamics(const std::array<float2, 4>& control_rngs, hipStream_t stream = 0) : PARENT_CLASS(stream)
  {
    for (int i = 0; i < CONTROL_DIM; i++)
      this->control_rngs_[i] = control_rngs[i];
    this->zero_control_[C_INDEX(THRUST)] = mppi::math::GRAVITY;
  }

  static const char* getDynamicsModelName()
  {
    return "Quadrotor Model";
  }

  /** at rest at the origin, level: the identity attitude (quadrotor_dynamics.cu:212-234) */
  state_array getZeroState() const
  {
    state_array zero;
    getZeroState(zero.data());
    return zero;
  }
  __host__ __device__ void getZeroState(float* state) const
  {
    for (int i = 0; i < STATE_DIM; i++)
      state[i] = (i == S_INDEX(QUAT_W)) ? 1.0f : 0.0f;
  }

  /**
   * quadrotor_dynamics.cu:127-173.  x_d = v;  v_d = (thrust / mass) * (body z axis in the world frame) - g e_z;
   * q_d = omega2edot(w, q);  w_d = (u_pqr - w) / tau.  The lanes of a rollout share the three-vectors by index; the lane that
   * owns v_d[2] subtracts gravity from its own product (the reference does it on lane 0 behind a block barrier: the same two
   * roundings), so no lane reads what another wrote and the method has no barrier of its own: where the reference has
   * __syncthreads() inside computeDynamics, the mppi::lane_sync() between computeStateDeriv and updateState in Dynamics::step
   * (plugin/dynamics.hpp) is the one that matters here.  Only the third column of the DCM is used,
   * and only that is computed.
   */
  __device__ inline void computeDynamics(float* state, float* control, float* state_der, float* theta = nullptr)
  {
    const float* v = state + S_INDEX(VEL_X);
    const float* q = state + S_INDEX(QUAT_W);
    const float* w = state + S_INDEX(ANG_VEL_X);
    float* x_d = state_der + S_INDEX(POS_X);
    float* v_d = state_der + S_INDEX(VEL_X);
    float* q_d = state_der + S_INDEX(QUAT_W);
    float* w_d = state_der + S_INDEX(ANG_VEL_X);

    float body_z[3];
    mppi::math::Quat2DCMColumn3(q, body_z);
    const float accel = control[C_INDEX(THRUST)] / this->params_.mass;

    int p_index, p_step;
    mppi::p1::getParallel1DIndex<mppi::p1::Parallel1Dir::THREAD_Y>(p_index, p_step);
    for (int i = p_index; i < 3; i += p_step)
    {
      x_d[i] = v[i];
      const float lift = accel * body_z[i];
      v_d[i] = (i == 2) ? lift - mppi::math::GRAVITY : lift;
    }
    // every lane writes the same seven values below, as in the reference
    mppi::math::omega2edot(w[0], w[1], w[2], q, q_d);
    w_d[0] = (control[C_INDEX(ANG_RATE_X)] - w[0]) / this->params_.tau_roll;
    w_d[1] = (control[C_INDEX(ANG_RATE_Y)] - w[1]) / this->params_.tau_pitch;
    w_d[2] = (control[C_INDEX(ANG_RATE_Z)] - w[2]) / this->params_.tau_yaw;
  }

  /**
   * Jacobians of computeDynamics at (state, control): A[13][13], B[13][4] row-major, zeroed by the caller (plugin/dynamics.hpp:
   * compute_grad).  Reference: QuadrotorDynamics::computeGrad, quadrotor_dynamics.cu:35-68, which fills d x_d / d v, d w_d / d w,
   * d v_d / d thrust and d w_d / d u, leaves the quaternion columns as TODOs, books d q_d / d w under B, and returns false.
   * Here every block of the derivative of computeDynamics as written above is filled, so the method returns true:
   *   d x_d / d v = I
   *   d v_d / d q = (thrust / mass) d(body z axis) / d q      d v_d / d thrust = (body z axis) / mass
   *   d q_d / d q, d q_d / d w: omega2edot is bilinear in (w, q), the entries are +-w_i / 2 and +-q_i / 2
   *   d w_d / d w = -1 / tau                                   d w_d / d u = 1 / tau
   * (the quaternion is not re-normalised inside computeDynamics, so none of that enters).
   */
  __host__ __device__ inline bool computeGrad(const float* state, const float* control, float* A, float* B) const
  {
    constexpr int NS = STATE_DIM, NC = CONTROL_DIM;
    constexpr int P0 = S_INDEX(POS_X), V0 = S_INDEX(VEL_X), Q0 = S_INDEX(QUAT_W), W0 = S_INDEX(ANG_VEL_X);
    const float* q = state + Q0;
    const float* w = state + W0;
    for (int i = 0; i < 3; i++)
      A[(P0 + i) * NS + V0 + i] = 1.0f;

    const float accel = control[C_INDEX(THRUST)] / this->params_.mass;
    // rows of d(body z axis) / d(q_w, q_x, q_y, q_z) over 2 (math_utils.hpp: Quat2DCMColumn3)
    const float dz[3][4] = { { q[2], q[3], q[0], q[1] }, { -q[1], -q[0], q[3], q[2] }, { q[0], -q[1], -q[2], q[3] } };
    float body_z[3];
    mppi::math::Quat2DCMColumn3(q, body_z);
    for (int i = 0; i < 3; i++)
    {
      for (int j = 0; j < 4; j++)
        A[(V0 + i) * NS + Q0 + j] = accel * (2 * dz[i][j]);
      B[(V0 + i) * NC + C_INDEX(THRUST)] = body_z[i] / this->params_.mass;
    }

    // q_d = 1/2 q x (0, w): rows by q_d component, columns by q component, then by body rate
    const float hw[3] = { 0.5f * w[0], 0.5f * w[1], 0.5f * w[2] };
    const float hq[4] = { 0.5f * q[0], 0.5f * q[1], 0.5f * q[2], 0.5f * q[3] };
    const float dq_dq[4][4] = { { 0.0f, -hw[0], -hw[1], -hw[2] },
                                { hw[0], 0.0f, hw[2], -hw[1] },
                                { hw[1], -hw[2], 0.0f, hw[0] },
                                { hw[2], hw[1], -hw[0], 0.0f } };
    const float dq_dw[4][3] = { { -hq[1], -hq[2], -hq[3] }, { hq[0], -hq[3], hq[2] }, { hq[3], hq[0], -hq[1] }, { -hq[2], hq[1], hq[0] } };
    for (int i = 0; i < 4; i++)
    {
      for (int j = 0; j < 4; j++)
        if (i != j)
          A[(Q0 + i) * NS + Q0 + j] = dq_dq[i][j];
      for (int j = 0; j < 3; j++)
        A[(Q0 + i) * NS + W0 + j] = dq_dw[i][j];
    }

    const float tau[3] = { this->params_.tau_roll, this->params_.tau_pitch, this->params_.tau_yaw };
    for (int i = 0; i < 3; i++)
    {
      A[(W0 + i) * NS + W0 + i] = -1.0f / tau[i];
      B[(W0 + i) * NC + C_INDEX(ANG_RATE_X) + i] = 1.0f / tau[i];
    }
    return true;
  }

  /**
   * quadrotor_dynamics.cu:175-188: the Euler step, then q /= |q| * copysign(1, q_w).
   *
   * The reference's device version lets every lane read next_state's quaternion for the norm and the sign while lane 0 may
   * already have divided q_w: a race with more than one lane per rollout.  Here each lane forms the four stepped quaternion
   * components itself from state and state_der, which nobody writes in this phase, takes norm and sign from those, and then
   * writes only the states it owns.  The result is the race-free one, and the one-lane form (where the compiler merges the
   * repeated products) computes exactly the same.
   *
   * With more than one lane this relies on the barrier Dynamics::step puts between computeStateDeriv and updateState: state_der
   * holds what OTHER lanes wrote (v_d, x_d by index).  A caller that runs updateState outside step() must place that
   * lane_sync() itself.  state and next_state are distinct buffers in every kernel.
   */
  __device__ inline void updateState(float* state, float* next_state, float* state_der, const float dt)
  {
    constexpr int Q0 = S_INDEX(QUAT_W);
    float q[4];
#pragma unroll
    for (int i = 0; i < 4; i++)
      q[i] = state[Q0 + i] + state_der[Q0 + i] * dt;
    const float q_norm = mppi::det::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const float scale = q_norm * mppi::det::copysign(1.0f, q[0]);

    int p_index, p_step;
    mppi::p1::getParallel1DIndex<mppi::p1::Parallel1Dir::THREAD_Y>(p_index, p_step);
    for (int i = p_index; i < STATE_DIM; i += p_step)
    {
      const float stepped = state[i] + state_der[i] * dt;
      next_state[i] = (i >= Q0 && i < Q0 + 4) ? stepped / scale : stepped;
    }
  }
};

#endif
