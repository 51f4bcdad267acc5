/**
 * CartpoleDynamics plugin (reference: include/mppi/dynamics/cartpole/cartpole_dynamics.cuh:6-105,
 * cartpole_dynamics.cu:89-107 — the device computeDynamics, expression for expression).
 * The reference's __sinf/__cosf become the bit-reproducible det::sincos (see det_math.h for why).
 */
#ifndef MPPI_AMD_CARTPOLE_DYNAMICS_HPP_
#define MPPI_AMD_CARTPOLE_DYNAMICS_HPP_

#include "mppi_amd/plugin/dynamics.hpp"

struct CartpoleDynamicsParams : public DynamicsParams
{
  enum class StateIndex : int
  {
    POS_X = 0,
    VEL_X,
    THETA,
    THETA_DOT,
    NUM_STATES
  };
  enum class ControlIndex : int
  {
    FORCE = 0,
    NUM_CONTROLS
  };
  enum class OutputIndex : int
  {
    POS_X = 0,
    VEL_X,
    THETA,
    THETA_DOT,
    NUM_OUTPUTS
  };
  float cart_mass = 1.0f;
  float pole_mass = 1.0f;
  float pole_length = 1.0f;

  CartpoleDynamicsParams() = default;
  CartpoleDynamicsParams(float cart_mass, float pole_mass, float pole_length)
    : cart_mass(cart_mass), pole_mass(pole_mass), pole_length(pole_length){};
};

using namespace MPPI_internal;

class CartpoleDynamics : public Dynamics<CartpoleDynamics, CartpoleDynamicsParams>
{
public:
  /** no block barrier in the per-step device methods: may run on the role-separated kernels (plugin/parallel_utils.hpp) */
  static constexpr bool MPPI_BARRIER_FREE_STEP = true;
  using PARENT_CLASS = Dynamics<CartpoleDynamics, CartpoleDynamicsParams>;
  CartpoleDynamics(float cart_mass = 1.0f, float pole_mass = 1.0f, float pole_length = 1.0f, hipStream_t stream = 0)
    : PARENT_CLASS(stream)
  {
    this->params_ = CartpoleDynamicsParams(cart_mass, pole_mass, pole_length);
  }

  static const char* getDynamicsModelName()
  {
    return "Cartpole Model";
  }
  __host__ __device__ float getCartMass()
  {
    return this->params_.cart_mass;
  };
  __host__ __device__ float getPoleMass()
  {
    return this->params_.pole_mass;
  };
  __host__ __device__ float getPoleLength()
  {
    return this->params_.pole_length;
  };
  __host__ __device__ float getGravity()
  {
    return gravity_;
  }

  __device__ inline void computeDynamics(float* state, float* control, float* state_der, float* theta = nullptr)
  {
    // reference: angle_utils::normalizeAngle(state[2]) (cartpole_dynamics.cu:91); the bounded variant returns the same
    // value for |theta| < 1e7 rad and keeps the range test off the rollout's dependent chain
    float theta_n = angle_utils::normalizeAngleBounded(state[2]);
    float sin_theta, cos_theta;
    mppi::det::sincos(theta_n, &sin_theta, &cos_theta);
    float theta_dot = state[3];
    float force = control[0];
    float m_c = this->params_.cart_mass;
    float m_p = this->params_.pole_mass;
    float l_p = this->params_.pole_length;

    state_der[0] = state[1];
    // 1.0f / x with x = m_c + m_p sin^2 and x = l_p (m_c + m_p sin^2): positive, ordinary magnitudes -> det::rcp_benign2
    // returns the correctly rounded IEEE reciprocals (what the reference's `1.0f / (...)` and the CPU oracle compute),
    // both in 8 instructions
    const float den = m_c + m_p * SQ(sin_theta);
    float r_x, r_th;
    mppi::det::rcp_benign2(den, l_p * den, &r_x, &r_th);
    state_der[1] = r_x * (force + m_p * sin_theta * (l_p * SQ(theta_dot) + gravity_ * cos_theta));
    state_der[2] = theta_dot;
    state_der[3] =
        r_th *
        (-force * cos_theta - m_p * l_p * SQ(theta_dot) * cos_theta * sin_theta - (m_c + m_p) * gravity_ * sin_theta);
  }

  /**
   * Continuous-time Jacobians of computeDynamics at (state, control): A[4][4] = d xdot / d x, B[4][1] = d xdot / d u, row-major,
   * zeroed by the caller (plugin/dynamics.hpp: compute_grad).  Reference: CartpoleDynamics::computeGrad, cartpole_dynamics.cu:10-46.
   * With s, c of the wrapped angle, w = theta_dot, den = m_c + m_p s^2 and lw2 = l_p w^2:
   *   d x_dd / d theta      = (m_p c (lw2 + g c) - g m_p s^2) / den - 2 m_p c s (F + m_p s (lw2 + g c)) / den^2
   *   d theta_dd / d theta  = (F s - g c (m_p + m_c) - l_p m_p w^2 c^2 + l_p m_p w^2 s^2) / (l_p den)
   *                           + 2 m_p c s (l_p m_p c s w^2 + F c + g s (m_p + m_c)) / (l_p den^2)
   * The numerator of the second line is a difference of near-equal terms around theta = +-pi/4 and the upright pole; its terms are
   * added left to right as the reference writes them.  The reference divides the last quotient by (l_p den)^2: one l_p too many,
   * invisible at its default l_p = 1; here it is the derivative of theta_dd as computeDynamics defines it.
   */
  __host__ __device__ inline bool computeGrad(const float* state, const float* control, float* A, float* B) const
  {
    float s, c;
    mppi::det::sincos(angle_utils::normalizeAngleBounded(state[2]), &s, &c);
    const float w = state[3];
    const float force = control[0];
    const float m_c = this->params_.cart_mass;
    const float m_p = this->params_.pole_mass;
    const float l_p = this->params_.pole_length;
    const float g = gravity_;
    const float den = m_c + m_p * SQ(s);
    const float swing = l_p * SQ(w) + g * c;  // l_p w^2 + g c
    const float m_total = m_p + m_c;

    A[0 * 4 + 1] = 1.0f;
    A[1 * 4 + 2] = (m_p * c * swing - g * m_p * SQ(s)) / den - (2 * m_p * c * s * (force + m_p * s * swing)) / SQ(den);
    A[1 * 4 + 3] = (2 * l_p * m_p * w * s) / den;
    A[2 * 4 + 3] = 1.0f;
    A[3 * 4 + 2] = (force * s - g * c * m_total - l_p * m_p * SQ(w) * SQ(c) + l_p * m_p * SQ(w) * SQ(s)) / (l_p * den) +
                   (2 * m_p * c * s * (l_p * m_p * c * s * SQ(w) + force * c + g * s * m_total)) / (l_p * SQ(den));
    A[3 * 4 + 3] = -(2 * m_p * w * c * s) / den;

    B[1] = 1 / den;
    B[3] = -c / (l_p * den);
    return true;
  }

  /* Split step (plugin/dynamics.hpp): only (theta, theta_dot) feed back — the cart's x and x_dot integrate values the angle
   * chain produces.  The core advances the angle pair; the completion, on the pipelined kernel's cost wave, rebuilds the cart
   * from sin, cos and the new theta_dot.  Both halves repeat computeDynamics' expressions and updateState's Euler step
   * operation for operation (fp contraction is off), so next state and output are step()'s bits. */
  using SPLIT_STEP_CLASS = CartpoleDynamics;
  static constexpr int SPLIT_CARRY = 3;  // theta_dot_{t+1}, sin(theta_t), cos(theta_t)

  __device__ inline void stepCore(const float* state, float* next_state, const float* control, float* carry, const float dt)
  {
    float theta_n = angle_utils::normalizeAngleBounded(state[2]);
    float sin_theta, cos_theta;
    mppi::det::sincos(theta_n, &sin_theta, &cos_theta);
    float theta_dot = state[3];
    float force = control[0];
    float m_c = this->params_.cart_mass;
    float m_p = this->params_.pole_mass;
    float l_p = this->params_.pole_length;
    const float den = m_c + m_p * SQ(sin_theta);
    // rcp_benign2's second lane alone: the same correctly rounded reciprocal; the first (the cart's) is the completion's
    const float r_th = mppi::det::rcp_benign(l_p * den);
    const float theta_dd =
        r_th *
        (-force * cos_theta - m_p * l_p * SQ(theta_dot) * cos_theta * sin_theta - (m_c + m_p) * gravity_ * sin_theta);
    next_state[2] = state[2] + theta_dot * dt;
    next_state[3] = theta_dot + theta_dd * dt;
    carry[0] = next_state[3];
    carry[1] = sin_theta;
    carry[2] = cos_theta;
  }

  __device__ inline void stepComplete(float* state, const float* control, const float* carry, float* output, const float dt)
  {
    const float sin_theta = carry[1], cos_theta = carry[2];
    float theta_dot = state[3];
    float force = control[0];
    float m_c = this->params_.cart_mass;
    float m_p = this->params_.pole_mass;
    float l_p = this->params_.pole_length;
    const float den = m_c + m_p * SQ(sin_theta);
    const float r_x = mppi::det::rcp_benign(den);
    const float x_dd = r_x * (force + m_p * sin_theta * (l_p * SQ(theta_dot) + gravity_ * cos_theta));
    state[0] = state[0] + state[1] * dt;
    state[1] = state[1] + x_dd * dt;
    state[2] = state[2] + theta_dot * dt;
    state[3] = carry[0];
#pragma unroll
    for (int i = 0; i < 4; i++)
      output[i] = state[i];
  }

protected:
  const float gravity_ = 9.81;
};

#endif
