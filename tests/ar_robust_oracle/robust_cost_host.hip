/**
 * robust_cost_host.hip — the HOST form of the shipped ARRobustCost (include/mppi_amd/cost_functions/autorally/ar_robust_cost.hpp,
 * __host__ __device__ in its three cost methods) and of its parameter class, exported for ctypes.  TEST CODE ONLY.  Compiled by
 * tests/ar_robust_oracle/__init__.py with hipcc for the host alone; tests/test_ar_robust_cost.py holds it to the reference's
 * known answers, to hand-derived answers and to the CPU restatement bit for bit.
 */
#include "mppi_amd/cost_functions/autorally/ar_robust_cost.hpp"
#include "mppi_amd/model_params.h"

#include <cstddef>
#include <cstring>

static_assert(sizeof(mppi_ar_robust_cost_params) == sizeof(ARRobustCostParams), "POD block and plugin parameters differ");
/* every field of the block, in order (ARRobustCostParams is not a standard-layout type — its bases hold fields too — so its
 * offsets are taken from an object, at run time: robust_cost_field_offsets) */
#define ROBUST_COST_FIELDS(X)                                                                                                  \
  X(control_cost_coeff) X(discount) X(desired_speed) X(speed_coeff) X(track_coeff) X(max_slip_ang) X(slip_coeff) X(track_slop) \
  X(crash_coeff) X(boundary_threshold) X(grid_res) X(r_c1) X(r_c2) X(trs) X(heading_coeff)

namespace
{
ARRobustCost& cost()
{
  static ARRobustCost c;
  return c;
}
}  // namespace

extern "C" {
/** the class's default parameters as the POD block */
void robust_cost_default_params(mppi_ar_robust_cost_params* out)
{
  const ARRobustCostParams d;
  memcpy(out, &d, sizeof(d));
}
/** byte offsets of the 15 fields in the plugin's class and in the POD block of model_params.h, then the two sizes; returns 15 */
int robust_cost_field_offsets(int* in_class, int* in_pod)
{
  const ARRobustCostParams d;
  int n = 0;
#define X(f)                                                \
  in_class[n] = (int)((const char*)&d.f - (const char*)&d); \
  in_pod[n++] = (int)offsetof(mppi_ar_robust_cost_params, f);
  ROBUST_COST_FIELDS(X)
#undef X
  in_class[n] = (int)sizeof(ARRobustCostParams);
  in_pod[n] = (int)sizeof(mppi_ar_robust_cost_params);
  return n;
}
void robust_cost_set_params(const mppi_ar_robust_cost_params* block)
{
  memcpy((void*)&cost().params_, block, sizeof(*block));
}
/** texels [height][width][4], 16-byte aligned, kept by the caller */
void robust_cost_set_costmap(const float* texels, int height, int width)
{
  cost().costmap_d_ = texels;
  cost().height_ = height;
  cost().width_ = width;
}
float robust_cost_state_cost(const float* s, int t, int* crash)
{
  return cost().computeStateCost(s, t, nullptr, crash);
}
/** out: the stabilizing cost and the costmap cost */
void robust_cost_terms(const float* s, float* out)
{
  out[0] = cost().getStabilizingCost(s);
  out[1] = cost().getCostmapCost(s);
}
int robust_cost_texel_index(float x, float y)
{
  return cost().texelIndexTransformed(x, y);
}
float robust_cost_max_cost_value()
{
  return ARRobustCost::MAX_COST_VALUE;
}
/** bit 0 MPPI_BARRIER_FREE_STEP, bit 1 MPPI_KERNARG_VIEWABLE; bits 4.. COSTMAP_CHANNELS */
int robust_cost_traits()
{
  return (ARRobustCost::MPPI_BARRIER_FREE_STEP ? 1 : 0) | (ARRobustCost::MPPI_KERNARG_VIEWABLE ? 2 : 0) |
         (ARRobustCost::COSTMAP_CHANNELS << 4);
}
}  // extern "C"
