/**
 * map_cost_host.hip — the HOST form of the shipped QuadrotorMapCost (include/mppi_amd/cost_functions/quadrotor/quadrotor_map_cost.hpp,
 * __host__ __device__ throughout) and of its parameter class, exported for ctypes.  TEST CODE ONLY.  Compiled by
 * tests/quadrotor_map_oracle/__init__.py with hipcc for the host alone; tests/test_quadrotor_map_cost.py holds it to hand-derived
 * answers and to the CPU restatement bit for bit.
 */
#include "mppi_amd/cost_functions/quadrotor/quadrotor_map_cost.hpp"
#include "mppi_amd/model_params.h"

#include <cstddef>
#include <cstring>

static_assert(sizeof(mppi_quadrotor_map_cost_params) == sizeof(QuadrotorMapCostParams), "POD block and plugin parameters differ");
/* every field of the block, in order (QuadrotorMapCostParams is not a standard-layout type — its base holds fields too — so its
 * offsets are taken from an object, at run time: map_cost_field_offsets) */
#define MAP_COST_FIELDS(X)                                                                                                     \
  X(control_cost_coeff) X(discount) X(r_c1) X(r_c2) X(trs) X(attitude_coeff) X(crash_coeff) X(dist_to_waypoint_coeff)          \
  X(heading_coeff) X(heading_power) X(height_coeff) X(track_coeff) X(speed_coeff) X(track_slop) X(gate_pass_cost)              \
  X(curr_waypoint) X(prev_waypoint) X(curr_gate_left) X(curr_gate_right) X(prev_gate_left) X(prev_gate_right) X(end_waypoint)  \
  X(desired_speed) X(gate_margin) X(min_dist_to_gate_side) X(track_boundary_cost) X(gate_width)

namespace
{
QuadrotorMapCost& cost()
{
  static QuadrotorMapCost c;
  return c;
}
}  // namespace

extern "C" {
/** the class's default parameters as the POD block */
void map_cost_default_params(mppi_quadrotor_map_cost_params* out)
{
  const QuadrotorMapCostParams d;
  memcpy(out, &d, sizeof(d));
}
/** byte offsets of the 27 fields in the plugin's class and in the POD block of model_params.h, then the two sizes; returns 27 */
int map_cost_field_offsets(int* in_class, int* in_pod)
{
  const QuadrotorMapCostParams d;
  int n = 0;
#define X(f)                                                         \
  in_class[n] = (int)((const char*)&d.f - (const char*)&d);          \
  in_pod[n++] = (int)offsetof(mppi_quadrotor_map_cost_params, f);
  MAP_COST_FIELDS(X)
#undef X
  in_class[n] = (int)sizeof(QuadrotorMapCostParams);
  in_pod[n] = (int)sizeof(mppi_quadrotor_map_cost_params);
  return n;
}
/** QuadrotorMapCostParams::updateWaypoint / updateGateBoundaries on a caller's block; returns whether it changed */
int map_cost_update_waypoint(mppi_quadrotor_map_cost_params* block, float x, float y, float z, float heading)
{
  QuadrotorMapCostParams p;
  memcpy((void*)&p, block, sizeof(p));
  const bool changed = p.updateWaypoint(x, y, z, heading);
  memcpy(block, &p, sizeof(p));
  return changed;
}
int map_cost_update_gate(mppi_quadrotor_map_cost_params* block, const float* lr)
{
  QuadrotorMapCostParams p;
  memcpy((void*)&p, block, sizeof(p));
  const bool changed = p.updateGateBoundaries(lr[0], lr[1], lr[2], lr[3], lr[4], lr[5]);
  memcpy(block, &p, sizeof(p));
  return changed;
}
void map_cost_set_params(const mppi_quadrotor_map_cost_params* block)
{
  memcpy((void*)&cost().params_, block, sizeof(*block));
}
/** values [height][width] (kept by the caller); frame: origin[3], rotations[9], resolution[3]; height == 0: no map */
void map_cost_set_costmap(const float* values, int height, int width, const float* frame)
{
  auto& tex = cost().tex_helper_.textures_[0];
  tex.use = height > 0 && width > 0;
  tex.data = tex.use ? values : nullptr;
  tex.height = height;
  tex.width = width;
  if (!tex.use)
    return;
  for (int i = 0; i < 3; i++)
    tex.origin[i] = frame[i];
  for (int i = 0; i < 9; i++)
    tex.rotations[i] = frame[3 + i];
  for (int i = 0; i < 3; i++)
    tex.resolution[i] = frame[12 + i];
}
float map_cost_state_cost(const float* s, int t, int* crash)
{
  float y[13];
  memcpy(y, s, sizeof(y));
  return cost().computeStateCost(y, t, nullptr, crash);
}
float map_cost_terminal_cost(const float* s)
{
  float y[13];
  memcpy(y, s, sizeof(y));
  return cost().terminalCost(y);
}
/** out: costmap, gate side, height, heading, speed, attitude, waypoint terms and the distance to the waypoint */
void map_cost_terms(const float* s, float* out)
{
  QuadrotorMapCost& c = cost();
  out[0] = c.computeCostmapCost(s);
  out[1] = c.computeGateSideCost(s);
  out[2] = c.computeHeightCost(s);
  out[3] = c.computeHeadingCost(s);
  out[4] = c.computeSpeedCost(s);
  out[5] = c.computeStabilizingCost(s);
  out[6] = c.computeWaypointCost(s);
  out[7] = c.distToWaypoint(s, c.params_.curr_waypoint);
}
float map_cost_max_cost_value()
{
  return QuadrotorMapCost::MAX_COST_VALUE;
}
int map_cost_traits()
{
  return (QuadrotorMapCost::MPPI_BARRIER_FREE_STEP ? 1 : 0) | (QuadrotorMapCost::MPPI_KERNARG_VIEWABLE ? 2 : 0);
}
}  // extern "C"
