/**
 * ar_robust_oracle.cpp — CPU restatement of ARRobustCost for the tests (tests/test_ar_robust_cost.py).  TEST CODE ONLY.
 *
 * The cost in plain C++ on the interfaces of oracle/oracle_core.hpp, with its own point sampler over a four-channel map, on the
 * oracle's ARNeuralNetModel (oracle/oracle_models.hpp, unchanged).  tests/ar_robust_oracle/__init__.py compiles this file TOGETHER
 * with oracle/oracle_capi.cpp into one library, so the handle ar_robust_oracle_create() returns is an oracle::Controller of that
 * library and every oracle_* entry point — the Vanilla, Tube and Robust loops among them — takes it.
 *
 * Restates the reference's device code (cost_functions/autorally/ar_robust_cost.cu:13-127) as one thread evaluates it, with the
 * plugin's documented choices: det:: transcendentals, one sincos of the yaw for both footprints and the heading term, the double
 * literals of the slip ramp and of `1.0 - boundary_threshold` kept.  It follows the plugin's ORDER OF ADDITIONS on purpose (0 ulp
 * against the kernels is the bar); what guards the formulas is the float64 restatement in the test file.
 */
#include "oracle_models.hpp"

#include <cstring>

namespace
{
namespace det = mppi::det;

/** which branches one evaluation took (ar_robust_census) */
struct Branches
{
  int constraint = 0;  ///< 0 below boundary_threshold, 1 on the ramp, 2 saturated at 1
  bool track_on = false, speed_from_map = false, heading_on = false;
  int slip = 0;  ///< 0 below the ramp, 1 on it, 2 saturated
  bool rolled = false, max_cost = false;
};

struct Texel
{
  float boundary, track, speed, heading;
};

struct ARRobustCost : oracle::Cost
{
  mppi_ar_robust_cost_params p;
  std::vector<Texel> map;
  int width = -1, height = -1;
  Branches last;
  static constexpr float MAX_COST_VALUE = 1e16f;

  ARRobustCost() : oracle::Cost(2, 8)
  {
    memset(&p, 0, sizeof(p));
    p.discount = 1.0f;
    p.desired_speed = -1.0f;
    p.speed_coeff = 20.0f;
    p.track_coeff = 33.0f;
    p.max_slip_ang = 1.5f;
    p.crash_coeff = 125000.0f;
    p.boundary_threshold = 0.75f;
    p.grid_res = 10;
    p.r_c1[0] = p.r_c2[1] = p.trs[2] = 1.0f;
  }
  int setParams(const void* pod, size_t n) override
  {
    if (n != sizeof(p))
      return -1;
    memcpy(&p, pod, n);
    return 0;
  }

  /** texel under a world position: normalised coordinates, floor, clamp to the map, NaN -> 0 */
  static int cell(float normalised, int size)
  {
    const float f = floorf(normalised * (float)size);
    if (!(f >= 0.0f))
      return 0;
    return f < (float)size ? (int)f : size - 1;
  }
  const Texel& sample(float x, float y) const
  {
    const float u = p.r_c1[0] * x + p.r_c2[0] * y + p.trs[0];
    const float v = p.r_c1[1] * x + p.r_c2[1] * y + p.trs[1];
    const float w = p.r_c1[2] * x + p.r_c2[2] * y + p.trs[2];
    return map[(size_t)cell(v / w, height) * width + cell(u / w, width)];
  }

  /** slip and roll: slip_coeff slip + penalty */
  float stabilizing(const float* s)
  {
    const bool standing = (double)fabsf(s[4]) < 0.001;
    const float slip = standing ? 0.0f : fabsf(-det::atan(s[5] / fabsf(s[4])));
    float penalty = 0.0f;
    last.slip = 0;
    if ((double)slip >= 0.75 * (double)p.max_slip_ang)
    {
      const float share = fminf(1.0f, slip / p.max_slip_ang);
      penalty = (float)(((double)share - 0.75) / (1.0 - 0.75)) * p.crash_coeff;
      last.slip = share < 1.0f ? 1 : 2;
    }
    last.rolled = (double)fabsf(s[3]) >= M_PI_2;
    if (last.rolled)
      penalty = p.crash_coeff;
    return p.slip_coeff * slip + penalty;
  }

  /** the four map terms, out[0..3] = constraint, track, speed, heading; returns their sum in the plugin's order */
  float costmap(const float* s, float* out)
  {
    float sin_yaw, cos_yaw;
    det::sincos(s[2], &sin_yaw, &cos_yaw);
    const Texel& front = sample(s[0] + 0.5f * cos_yaw, s[1] + 0.5f * sin_yaw);
    const Texel& back = sample(s[0] + -0.5f * cos_yaw, s[1] + -0.5f * sin_yaw);
    const float constraint = fminf(1.0f, fmaxf(front.boundary, back.boundary));
    out[0] = out[1] = 0.0f;
    last.constraint = 0;
    if (constraint >= p.boundary_threshold)
    {
      out[0] = (float)((double)(constraint - p.boundary_threshold) / (1.0 - (double)p.boundary_threshold)) * p.crash_coeff;
      last.constraint = constraint < 1.0f ? 1 : 2;
    }
    last.track_on = front.track > p.track_slop;
    if (last.track_on)
      out[1] = p.track_coeff * front.track;
    last.speed_from_map = p.desired_speed == -1;
    out[2] = p.speed_coeff * fabsf(s[4] - (last.speed_from_map ? front.speed : p.desired_speed));
    out[3] = p.heading_coeff * fabsf(sin_yaw + front.heading);
    last.heading_on = out[3] != 0.0f;
    float total = 0.0f;
    if (last.constraint)
      total += out[0];
    if (last.track_on)
      total += out[1];
    total += out[2];
    total += out[3];
    return total;
  }

  float computeStateCost(const float* s, int t, int* crash) override
  {
    float terms[4];
    const float stab = stabilizing(s);
    float total = stab + costmap(s, terms);
    last.max_cost = total > MAX_COST_VALUE || std::isnan(total);
    if (last.max_cost)
      total = MAX_COST_VALUE;
    return total;
  }
  float terminalCost(const float* s) override
  {
    return 0.0f;
  }
};

ARRobustCost* robustCost(void* h)
{
  return static_cast<ARRobustCost*>(((oracle::Controller*)h)->cost.get());
}
}  // namespace

extern "C" {
/** an oracle::Controller on the oracle's ARNeuralNetModel + ARRobustCost: every oracle_* entry point of this library takes it
 *  ("dynamics_weights" through oracle_set_blob; the map through ar_robust_set_costmap) */
void* ar_robust_oracle_create(int K, int T, int D, float dt, float lambda, float alpha, int num_iters)
{
  auto* c = new oracle::Controller();
  c->dyn.reset(new oracle::ARNeuralNetModel());
  c->cost.reset(new ARRobustCost());
  c->dt = dt;
  c->lambda = lambda;
  c->alpha = alpha;
  c->num_iters = num_iters;
  c->init(K, T, D);
  return c;
}

/** texels [height][width][4] */
void ar_robust_set_costmap(void* h, const float* texels, int height, int width)
{
  ARRobustCost* c = robustCost(h);
  c->map.resize((size_t)height * width);
  memcpy(c->map.data(), texels, c->map.size() * sizeof(Texel));
  c->height = height;
  c->width = width;
}

/** out: stabilizing cost, constraint, track, speed and heading terms, the costmap cost (their sum in the plugin's order) */
void ar_robust_terms(void* h, const float* s, float* out)
{
  ARRobustCost* c = robustCost(h);
  out[0] = c->stabilizing(s);
  out[5] = c->costmap(s, out + 1);
}

/**
 * Rolls the K rollouts of clamped controls v[K][T][2] out from x0 as oracle::rolloutCosts does and counts, over all rollout-steps,
 * the branches the cost took: counts[0..2] constraint below the threshold / on the ramp / saturated, [3..4] track term on / off,
 * [5..6] speed from the map / from desired_speed, [7] heading term non-zero, [8..10] slip below the ramp / on it / saturated,
 * [11] roll at or beyond pi/2, [12] MAX_COST_VALUE.
 */
void ar_robust_census(void* h, const float* x0, const float* v, int K, int T, int* counts)
{
  auto* ctl = (oracle::Controller*)h;
  ARRobustCost* c = robustCost(h);
  for (int i = 0; i < 13; i++)
    counts[i] = 0;
  std::vector<float> x(7), xn(7), xdot(7), u(2), y(8), theta(1);
  for (int k = 0; k < K; k++)
  {
    std::copy(x0, x0 + 7, x.begin());
    std::fill(xdot.begin(), xdot.end(), 0.0f);
    std::fill(y.begin(), y.end(), 0.0f);
    std::fill(u.begin(), u.end(), 0.0f);
    int crash = 0;
    ctl->dyn->initializeDynamics(x.data(), u.data(), y.data(), theta.data(), 0.0f, ctl->dt);
    for (int t = 0; t < T; t++)
    {
      std::copy(v + ((size_t)k * T + t) * 2, v + ((size_t)k * T + t) * 2 + 2, u.begin());
      ctl->dyn->enforceConstraints(x.data(), u.data());
      ctl->dyn->step(x.data(), xn.data(), xdot.data(), u.data(), y.data(), theta.data(), t, ctl->dt);
      (void)c->computeStateCost(y.data(), t, &crash);
      const Branches& b = c->last;
      counts[b.constraint]++;
      counts[b.track_on ? 3 : 4]++;
      counts[b.speed_from_map ? 5 : 6]++;
      counts[7] += b.heading_on;
      counts[8 + b.slip]++;
      counts[11] += b.rolled;
      counts[12] += b.max_cost;
      std::swap(x, xn);
    }
  }
}
}  // extern "C"
