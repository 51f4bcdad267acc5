/**
 * quadrotor_map_oracle.cpp — CPU restatement of QuadrotorMapCost for the tests (tests/test_quadrotor_map_cost.py).  TEST CODE ONLY.
 *
 * The cost in plain C++ on the interfaces of oracle/oracle_core.hpp, with the map looked up through oracle/oracle_texture.hpp;
 * the dynamics, the quaternion helpers and the arithmetic flavour are those of tests/quadrotor_oracle/quadrotor_oracle.cpp, which
 * this file includes as it stands.  tests/quadrotor_map_oracle/__init__.py compiles this file TOGETHER with oracle/oracle_capi.cpp
 * into one library, so the handle quadrotor_map_oracle_create() returns is an oracle::Controller of that library.
 *
 * Restates the reference's device code (cost_functions/quadrotor/quadrotor_map_cost.cu:93-144, 199-395) as one thread evaluates
 * it, in the straight-line order — map first — and with the plugin's documented choices: det:: transcendentals, the double
 * constants of the height term kept, no printf, a NaN sum is MAX_COST_VALUE.  It follows the plugin's ORDER OF ADDITIONS on
 * purpose (0 ulp against the kernels is the bar); what guards the formulas is the float64 restatement in the test file.
 */
#include "../quadrotor_oracle/quadrotor_oracle.cpp"
#include "oracle_texture.hpp"

namespace
{
struct Vec2
{
  float x, y;
};
inline Vec2 operator-(Vec2 a, Vec2 b)
{
  return Vec2{ a.x - b.x, a.y - b.y };
}
inline float dot(Vec2 a, Vec2 b)
{
  return a.x * b.x + a.y * b.y;
}
inline float cross(Vec2 a, Vec2 b)
{
  return a.x * b.y - a.y * b.x;
}
inline float length(Vec2 a)
{
  return det::sqrt(sq(a.x) + sq(a.y));
}

/** which branches one evaluation took (quadrotor_map_census) */
struct Branches
{
  bool left_map = false, off_track = false, gate_hit = false, gate_passed = false, heading_on = false, height_400 = false;
};

struct QuadrotorMapCost : oracle::Cost
{
  mppi_quadrotor_map_cost_params p;
  oracle::Texture2D map;
  std::vector<float> map_values;
  bool map_in_use = false;
  Branches last;

  QuadrotorMapCost() : oracle::Cost(4, 13)
  {
    memset(&p, 0, sizeof(p));
    for (float& c : p.control_cost_coeff)
      c = 1.0f;
    p.discount = 1.0f;
    p.r_c1[0] = p.r_c2[1] = p.trs[2] = 1.0f;
    p.attitude_coeff = 10.0f;
    p.crash_coeff = 1000.0f;
    p.heading_coeff = 5.0f;
    p.heading_power = 1.0f;
    p.height_coeff = 5.0f;
    p.track_coeff = 10.0f;
    p.speed_coeff = 5.0f;
    p.gate_pass_cost = -150.0f;
    for (float& c : p.end_waypoint)
      c = NAN;
    p.desired_speed = 5.0f;
    p.gate_margin = 0.5f;
    p.min_dist_to_gate_side = 0.5f;
    p.track_boundary_cost = 2.5f;
    p.gate_width = 2.15f;
  }
  int setParams(const void* pod, size_t n) override
  {
    if (n != sizeof(p))
      return -1;
    memcpy(&p, pod, n);
    return 0;
  }

  Vec2 position(const float* s) const
  {
    return Vec2{ s[0], s[1] };
  }
  float distanceToWaypoint(const float* s) const
  {
    return det::sqrt(sq(s[0] - p.curr_waypoint[0]) + sq(s[1] - p.curr_waypoint[1]) + sq(s[2] - p.curr_waypoint[2]));
  }

  float mapTerm(const float* s)
  {
    if (!map_in_use)
      return 0.0f;
    float in_map[3], uv[3], value = 0.0f;
    map.worldToMap(s, in_map);
    map.mapToTex(in_map, uv);
    float total = 0.0f;
    last.left_map = uv[0] < 0.0f || uv[0] > 1.0f || uv[1] < 0.0f || uv[1] > 1.0f;
    if (last.left_map)
      total += p.crash_coeff;
    map.query(uv, &value);
    if (value > p.track_slop)
      total += p.track_coeff * value;
    last.off_track = value > p.track_boundary_cost;
    if (last.off_track)
      total += p.crash_coeff;
    return total;
  }
  float gateSideTerm(const float* s)
  {
    const Vec2 left{ p.curr_gate_left[0], p.curr_gate_left[1] }, right{ p.curr_gate_right[0], p.curr_gate_right[1] };
    const Vec2 gate = left - right, from_right = position(s) - right;
    const float off_line = cross(from_right, gate);
    const float along = dot(from_right, gate) / dot(gate, gate);
    const bool before_right = along < 0.0f && along >= -0.5f, beyond_left = along > 1.0f && along <= 1.5f;
    last.gate_hit = fabsf(off_line) < p.min_dist_to_gate_side && (before_right || beyond_left);
    return last.gate_hit ? p.crash_coeff * fabsf(along) : 0.0f;
  }
  float heightTerm(const float* s)
  {
    const float from_prev = length(position(s) - Vec2{ p.prev_waypoint[0], p.prev_waypoint[1] });
    const float to_curr = length(position(s) - Vec2{ p.curr_waypoint[0], p.curr_waypoint[1] });
    // the reference's double constants: the denominator, both quotients and the blend are fp64, rounded at each float
    const double span = (double)(from_prev + to_curr) + 0.001;
    const float share_prev = (float)((double)from_prev / span), share_curr = (float)((double)to_curr / span);
    const float wanted =
        (float)((1.0 - (double)share_prev) * (double)p.prev_waypoint[2] + (1.0 - (double)share_curr) * (double)p.curr_waypoint[2]);
    const float miss = sq(fabsf(s[2] - wanted));
    float total = miss < 0 ? p.crash_coeff * (1 - miss) : p.height_coeff * miss;
    last.height_400 = miss > p.gate_width;
    if (last.height_400)
      total += 400;
    return total;
  }
  float headingTerm(const float* s)
  {
    float R[9];
    rotationMatrix(load(s + 6), R);
    const float flight_x = R[0] * s[3] + R[1] * s[4] + R[2] * s[5], flight_y = R[3] * s[3] + R[4] * s[4] + R[5] * s[5];
    const float flight_dir = det::atan2(flight_y, flight_x);
    const float bearing = det::atan2(p.curr_waypoint[1] - s[1], p.curr_waypoint[0] - s[0]);
    last.heading_on = distanceToWaypoint(s) > p.gate_margin;
    if (!last.heading_on)
      return 0.0f;
    const float off = fabsf(det::normalizeAngle(flight_dir - bearing));
    // powf's values at the two powers where exp(power * log(off)) is not needed or (off == 0, power == 0) has none
    const float raised = p.heading_power == 1.0f ? off : p.heading_power == 0.0f ? 1.0f : det::pow_pos(off, p.heading_power);
    return p.heading_coeff * raised;
  }
  float speedTerm(const float* s) const
  {
    return p.speed_coeff * sq(det::sqrt(s[3] * s[3] + s[4] * s[4]) - p.desired_speed);
  }
  float levelTerm(const float* s) const
  {
    float rpy[3];
    eulerAngles(load(s + 6), rpy);
    return p.attitude_coeff * (sq(rpy[0]) + sq(rpy[1]));
  }
  float waypointTerm(const float* s) const
  {
    return p.dist_to_waypoint_coeff * sq(distanceToWaypoint(s));
  }

  float computeStateCost(const float* s, int t, int* crash) override
  {
    const float on_map = mapTerm(s), gate = gateSideTerm(s), height = heightTerm(s), heading = headingTerm(s);
    const float speed = speedTerm(s), level = levelTerm(s);
    if (gate != 0)
      *crash = 1;
    float total = 0;
    total += on_map + gate + height + heading + speed + level;  // the waypoint term is not part of the device sum
    last.gate_passed = distanceToWaypoint(s) < p.gate_margin;
    if (last.gate_passed)
      total += p.gate_pass_cost;
    total += *crash * p.crash_coeff;
    return std::isnan(total) ? MAX_COST_VALUE : total;
  }
  float terminalCost(const float* s) override
  {
    return 0.0f;
  }
};

QuadrotorMapCost* mapCost(void* h)
{
  return static_cast<QuadrotorMapCost*>(((oracle::Controller*)h)->cost.get());
}
}  // namespace

extern "C" {
/** an oracle::Controller on QuadrotorDynamics + QuadrotorMapCost: every oracle_* entry point of this library takes it */
void* quadrotor_map_oracle_create(int K, int T, int D, float dt, float lambda, float alpha, int num_iters)
{
  auto* c = new oracle::Controller();
  c->dyn.reset(new QuadrotorDynamics());
  c->cost.reset(new QuadrotorMapCost());
  c->dt = dt;
  c->lambda = lambda;
  c->alpha = alpha;
  c->num_iters = num_iters;
  c->init(K, T, D);
  return c;
}

/** values [height][width]; frame: origin[3], rotations[9] row-major, resolution[3]; height == 0 takes the map away */
void quadrotor_map_set_costmap(void* h, const float* values, int height, int width, const float* frame)
{
  QuadrotorMapCost* c = mapCost(h);
  c->map_in_use = height > 0 && width > 0;
  if (!c->map_in_use)
    return;
  c->map_values.assign(values, values + (size_t)height * width);
  c->map.values = c->map_values.data();
  c->map.height = height;
  c->map.width = width;
  for (int i = 0; i < 3; i++)
  {
    c->map.origin[i] = frame[i];
    c->map.resolution[i] = frame[12 + i];
    for (int j = 0; j < 3; j++)
      c->map.rot[i][j] = frame[3 + 3 * i + j];
  }
}

/** out: costmap, gate side, height, heading, speed, attitude, waypoint terms and the distance to the waypoint */
void quadrotor_map_terms(void* h, const float* s, float* out)
{
  QuadrotorMapCost* c = mapCost(h);
  out[0] = c->mapTerm(s);
  out[1] = c->gateSideTerm(s);
  out[2] = c->heightTerm(s);
  out[3] = c->headingTerm(s);
  out[4] = c->speedTerm(s);
  out[5] = c->levelTerm(s);
  out[6] = c->waypointTerm(s);
  out[7] = c->distanceToWaypoint(s);
}

/**
 * Rolls the K rollouts of clamped controls v[K][T][4] out from x0 as oracle::rolloutCosts does and counts, over all rollout-steps,
 * the branches the cost took: counts = left the map, map value above track_boundary_cost, gate-side hit, gate passed, heading
 * term on, heading term off, the +400 height branch.  first_crash[k] is the step on which rollout k's crash flag was set, or -1.
 */
void quadrotor_map_census(void* h, const float* x0, const float* v, int K, int T, int* counts, int* first_crash)
{
  auto* ctl = (oracle::Controller*)h;
  QuadrotorMapCost* c = mapCost(h);
  for (int i = 0; i < 7; i++)
    counts[i] = 0;
  std::vector<float> x(13), xn(13), xdot(13), u(4), y(13), theta(1);
  for (int k = 0; k < K; k++)
  {
    std::copy(x0, x0 + 13, x.begin());
    std::fill(xdot.begin(), xdot.end(), 0.0f);
    int crash = 0;
    first_crash[k] = -1;
    for (int t = 0; t < T; t++)
    {
      std::copy(v + ((size_t)k * T + t) * 4, v + ((size_t)k * T + t) * 4 + 4, u.begin());
      ctl->dyn->enforceConstraints(x.data(), u.data());
      ctl->dyn->step(x.data(), xn.data(), xdot.data(), u.data(), y.data(), theta.data(), t, ctl->dt);
      (void)c->computeStateCost(y.data(), t, &crash);
      const Branches& b = c->last;
      const bool taken[7] = { b.left_map, b.off_track, b.gate_hit, b.gate_passed, b.heading_on, !b.heading_on, b.height_400 };
      for (int i = 0; i < 7; i++)
        counts[i] += taken[i];
      if (crash && first_crash[k] < 0)
        first_crash[k] = t;
      std::swap(x, xn);
    }
  }
}
}  // extern "C"
