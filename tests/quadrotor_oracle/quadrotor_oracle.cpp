/**
 * quadrotor_oracle.cpp — CPU restatement of the quadrotor model for the tests (tests/test_quadrotor.py).  TEST CODE ONLY.
 *
 * QuadrotorDynamics and QuadrotorQuadraticCost in plain C++ on the interfaces of oracle/oracle_core.hpp, so that the generic
 * machinery there — rolloutCosts, the Vanilla and Tube computeControl, slide, the state trajectory — applies unchanged.
 * tests/quadrotor_oracle/__init__.py compiles this file TOGETHER with oracle/oracle_capi.cpp into one library: the handle
 * quadrotor_oracle_create() returns is an oracle::Controller, and every oracle_* entry point of that library takes it.
 *
 * Restates the reference's device code (dynamics/quadrotor/quadrotor_dynamics.cu:127-188,
 * cost_functions/quadrotor/quadrotor_quadratic_cost.cu:70-133, utils/math_utils.h:166-283 and 534-540), as one thread with
 * blockDim.y == 1 evaluates it, in the arithmetic flavour the plugin documents (include/mppi_amd/plugin/math_utils.hpp): norms
 * are det::sqrt and a true division, the angles det::atan2 / det::asin, powf(x, 2) is x * x.  The transcendentals are shared
 * with the plugin on purpose (det_math.h, bounded by tests/test_det_math.py and the atan2 test); the float64 numpy restatement
 * in tests/test_quadrotor.py shares nothing with either.
 *
 * Independence: this file follows the plugin's ORDER OF OPERATIONS on purpose (the Euler terms enter the cost sum first, gravity
 * is subtracted from the product) — that is what makes 0 ulp against the kernels a meaningful bar, and it also means a mistake
 * in the formulas could be common to both.  What guards against that is the float64 restatement alone, at 1e-4.
 */
#include "oracle_core.hpp"
#include "mppi_amd/det_math.h"
#include "mppi_amd/model_params.h"

namespace
{
namespace det = mppi::det;
constexpr float GRAVITY = 9.81f;        // utils/math_utils.h:45
constexpr float MAX_COST_VALUE = 1e16f;  // quadrotor_quadratic_cost.cuh:93

inline float sq(float a)
{
  return a * a;
}

/* quaternions are (w, x, y, z); every sum below is left to right, which is the reference's order of operations */
struct Quat
{
  float w, x, y, z;
};
inline Quat load(const float* a)
{
  return Quat{ a[0], a[1], a[2], a[3] };
}
inline void store(const Quat& q, float* a)
{
  a[0] = q.w;
  a[1] = q.x;
  a[2] = q.y;
  a[3] = q.z;
}
inline float invNorm(const Quat& q)
{
  return 1.0f / det::sqrt(sq(q.w) + sq(q.x) + sq(q.y) + sq(q.z));
}
inline Quat scaled(const Quat& q, float k)
{
  return Quat{ q.w * k, q.x * k, q.y * k, q.z * k };
}
/** unit-length Hamilton product a x b */
Quat multiply(const Quat& a, const Quat& b)
{
  Quat c;
  c.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
  c.x = a.x * b.w + a.w * b.x - a.z * b.y + a.y * b.z;
  c.y = a.y * b.w + a.z * b.x + a.w * b.y - a.x * b.z;
  c.z = a.z * b.w - a.y * b.x + a.x * b.y + a.w * b.z;
  return scaled(c, invNorm(c));
}
Quat inverse(const Quat& q)
{
  const float k = invNorm(q);
  return Quat{ q.w * k, -q.x * k, -q.y * k, -q.z * k };
}
/** the rotation from `from` to `to` */
Quat difference(const Quat& from, const Quat& to)
{
  return multiply(to, inverse(from));
}
/** out = (roll, pitch, yaw) of the 3-2-1 sequence, NWU */
void eulerAngles(const Quat& q, float out[3])
{
  out[0] = det::atan2(2.0f * q.z * q.y + 2.0f * q.w * q.x, q.w * q.w + q.z * q.z - q.y * q.y - q.x * q.x);
  const float sin_pitch = -2.0f * q.w * q.y + 2.0f * q.x * q.z;
  out[1] = -det::asin(fmaxf(fminf(1.0f, sin_pitch), -1.0f));
  out[2] = det::atan2(2.0f * q.y * q.x + 2.0f * q.z * q.w, q.w * q.w + q.x * q.x - q.y * q.y - q.z * q.z);
}
/** body-to-world rotation matrix, row-major */
void rotationMatrix(const Quat& q, float R[9])
{
  R[0] = sq(q.w) + sq(q.x) - sq(q.y) - sq(q.z);
  R[1] = 2 * (q.x * q.y - q.w * q.z);
  R[2] = 2 * (q.x * q.z + q.w * q.y);
  R[3] = 2 * (q.x * q.y + q.w * q.z);
  R[4] = sq(q.w) - sq(q.x) + sq(q.y) - sq(q.z);
  R[5] = 2 * (q.y * q.z - q.w * q.x);
  R[6] = 2 * (q.x * q.z - q.w * q.y);
  R[7] = 2 * (q.y * q.z + q.w * q.x);
  R[8] = sq(q.w) - sq(q.x) - sq(q.y) + sq(q.z);
}
/** quaternion rate for body rates (p, q, r) */
Quat rate(float p, float q, float r, const Quat& e)
{
  return Quat{ 0.5f * (-p * e.x - q * e.y - r * e.z), 0.5f * (p * e.w - q * e.z + r * e.y), 0.5f * (p * e.z + q * e.w - r * e.x),
               0.5f * (-p * e.y + q * e.x + r * e.w) };
}

struct QuadrotorDynamics : oracle::Dynamics
{
  mppi_quadrotor_dynamics_params p{ 0.25f, 0.25f, 0.25f, 1.0f };
  QuadrotorDynamics() : oracle::Dynamics(13, 4, 13)
  {
    rng_lo[3] = 0.0f;  // quadrotor_dynamics.cu:11-19
    rng_hi[3] = 36.0f;
    zero_control[3] = GRAVITY;
  }
  int setParams(const void* pod, size_t n) override
  {
    if (n != sizeof(p))
      return -1;
    memcpy(&p, pod, n);
    return 0;
  }
  void computeDynamics(const float* state, const float* control, float* state_der, float* theta_s) override
  {
    const Quat attitude = load(state + 6);
    const float* rates = state + 10;
    float R[9];
    rotationMatrix(attitude, R);
    for (int axis = 0; axis < 3; axis++)
    {
      state_der[axis] = state[3 + axis];
      state_der[3 + axis] = (control[3] / p.mass) * R[3 * axis + 2];
    }
    state_der[5] -= GRAVITY;
    store(rate(rates[0], rates[1], rates[2], attitude), state_der + 6);
    const float tau[3] = { p.tau_roll, p.tau_pitch, p.tau_yaw };
    for (int axis = 0; axis < 3; axis++)
      state_der[10 + axis] = (control[axis] - rates[axis]) / tau[axis];
  }
  /** Euler, then q /= |q| * copysign(1, q_w) with norm and sign taken before any component is divided */
  void updateState(const float* x, float* x_next, const float* xdot, float dt) const override
  {
    oracle::Dynamics::updateState(x, x_next, xdot, dt);
    float* q = x_next + 6;
    const float q_norm = det::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const float sign = det::copysign(1.0f, q[0]);
    for (int i = 0; i < 4; i++)
      q[i] /= q_norm * sign;
  }
};

struct QuadrotorQuadraticCost : oracle::Cost
{
  mppi_quadrotor_cost_params params_{ { 2.0f, 2.0f, 2.0f, 2.0f }, 1.0f, { 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0 }, 1.0f, 1.0f, 1,
                                      1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 0.0f };
  QuadrotorQuadraticCost() : oracle::Cost(4, 13)
  {
  }
  int setParams(const void* pod, size_t n) override
  {
    if (n != sizeof(params_))
      return -1;
    memcpy(&params_, pod, n);
    return 0;
  }
  float computeStateCost(const float* s, int t, int* crash) override
  {
    /* the thirteen per-state terms first, as the reference fills its array; added up only after the attitude angles */
    float term[13];
    for (int i = 0; i < 13; i++)
    {
      const float weight = i < 3 ? params_.x_coeff : (i < 6 ? params_.v_coeff : (i < 10 ? 0.0f : params_.w_coeff));
      term[i] = sq(s[i] - params_.s_goal[i]) * weight;
    }
    float attitude_error[4];
    store(difference(load(s + 6), load(params_.s_goal + 6)), attitude_error);
    float total = 0;
    if (params_.use_euler)
    {
      float rpy[3];
      eulerAngles(load(attitude_error), rpy);
      total += params_.roll_coeff * sq(rpy[0]);
      total += params_.pitch_coeff * sq(rpy[1]);
      total += params_.yaw_coeff * sq(rpy[2]);
    }
    for (int i = 6; i < 10; i++)  // not squared without use_euler: the reference's device code (quadrotor_quadratic_cost.cu:93-99)
      term[i] = params_.use_euler ? 0.0f : params_.q_coeff * attitude_error[i - 6];
    for (int i = 0; i < 13; i++)
      total += term[i];
    return std::isnan(total) ? MAX_COST_VALUE : total;  // the plugin's deliberate fix of the reference's NaN guard
  }
  float terminalCost(const float* s) override
  {
    const float cost = params_.terminal_cost_coeff * computeStateCost(s, 0, nullptr);
    return std::isnan(cost) ? MAX_COST_VALUE : cost;
  }
};
}  // namespace

extern "C" {
/** an oracle::Controller on the quadrotor model: every oracle_* entry point of this library takes it; oracle_destroy frees it */
void* quadrotor_oracle_create(int K, int T, int D, float dt, float lambda, float alpha, int num_iters)
{
  auto* c = new oracle::Controller();
  c->dyn.reset(new QuadrotorDynamics());
  c->cost.reset(new QuadrotorQuadraticCost());
  c->dt = dt;
  c->lambda = lambda;
  c->alpha = alpha;
  c->num_iters = num_iters;
  c->init(K, T, D);
  return c;
}

float quadrotor_terminal_cost(void* h, const float* y)
{
  return ((oracle::Controller*)h)->cost->terminalCost(y);
}

void quadrotor_det_atan2(const float* y, const float* x, float* out, int n)
{
  for (int i = 0; i < n; i++)
    out[i] = det::atan2(y[i], x[i]);
}

/** the quaternion helpers on float arrays: 0 QuatMultiply(in[0:4], in[4:8]) -> out[4];  1 QuatInv(in[0:4]) -> out[4];
 *  2 QuatSubtract(in[0:4], in[4:8]) -> out[4];  3 Quat2EulerNWU(in[0:4]) -> out[3] (roll, pitch, yaw);
 *  4 Quat2DCM(in[0:4]) -> out[9] row-major;  5 omega2edot(in[0], in[1], in[2], in[3:7]) -> out[4] */
int quadrotor_quat_eval(int which, const float* in, float* out)
{
  switch (which)
  {
    case 0: store(multiply(load(in), load(in + 4)), out); return 4;
    case 1: store(inverse(load(in)), out); return 4;
    case 2: store(difference(load(in), load(in + 4)), out); return 4;
    case 3: eulerAngles(load(in), out); return 3;
    case 4: rotationMatrix(load(in), out); return 9;
    case 5: store(rate(in[0], in[1], in[2], load(in + 3)), out); return 4;
  }
  return -1;
}
}  // extern "C"
