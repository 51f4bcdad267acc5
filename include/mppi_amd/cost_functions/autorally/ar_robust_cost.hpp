/**
 * ARRobustCost — the AutoRally cost the reference pairs with Robust MPPI: boundary constraint, track position, speed map and
 * heading, read from ALL FOUR channels of the track map, plus a slip / roll penalty.
 * reference: include/mppi/cost_functions/autorally/ar_robust_cost.cuh:6-29 (parameters), ar_robust_cost.cu:13-37
 * (getStabilizingCost), :39-112 (getCostmapCost, the __CUDA_ARCH__ branch), :114-127 (computeStateCost).
 *
 * Costmap: the reference's float4 CUDA texture (point filter, clamp, normalised coordinates) with .x the boundary constraint,
 * .y the track position, .z the speed map and .w the heading.  Here it is a plain `float[height][width][4]` array in HBM, 16-byte
 * aligned, one texel = one 16-byte load; the texel is chosen by the rule ARStandardCost::queryTextureTransformed states
 * (floor(u * width), floor(v * height), clamped, NaN -> 0).  COSTMAP_CHANNELS tells the engine which "costmap" blob the class
 * takes: {height, width, 4}, interleaved texels (engine/model_traits.hpp: costmap_channels; engine/model_blobs.hpp: checkMapDims).
 *
 * The DEVICE branch is restated (the project's rule), on the host as on the device.  Kept as the reference has them:
 *   - the double literals of getStabilizingCost promote to fp64: `slip >= 0.75 * max_slip_ang` compares in double, and the ramp
 *     `(slip_val - 0.75) / (1.0 - 0.75)` is a double subtraction and a double division, rounded to float once;
 *     `fabs(roll) >= M_PI_2` and `fabs(vx) < 0.001` compare in double too.  Three fp64 operations per step;
 *   - `(constraint - boundary_threshold) / (1.0 - boundary_threshold)`: the numerator is a float subtraction, `1.0 - threshold`
 *     and the division are double;
 *   - boundary_threshold == 1 with a constraint of 1 is 0 / 0: the step costs MAX_COST_VALUE (computeStateCost's NaN rule);
 *   - the roll penalty REPLACES the slip ramp's, it is not added to it;
 *   - this cost never writes crash_status, and the discount is not applied to any of its terms.
 * What differs, on purpose:
 *   - transcendentals are mppi::det:: (atan, sincos);
 *   - one det::sincos of the yaw serves both footprints and the heading term; the reference evaluates __sinf twice and sinf once
 *     more for the heading (three sines that may differ in the last bits there; one value here);
 *   - the reference's host branch (round(u * width - 0.5)) is not restated.
 *
 * The texel fetch (getCostmapCost): both texel indices are computed first, both texels are loaded, and only then is the first
 * component used, so the two loads' latencies overlap instead of adding up in the wave's dependent chain (in the gfx950 code: two
 * loads back to back in front of one s_waitcnt; the front texel is one 16-byte load, the back texel — only .x is read — is
 * narrowed by the compiler to a 4-byte load; DESIGN.md, "AutoRally robust cost").  The two texels are
 * combined as VALUES (fmaxf of the two .x); the code never forms `cond ? front_address : back_address`, and no device method
 * stores to a member, so a role loop may run the class off the kernel's argument block (MPPI_KERNARG_VIEWABLE).
 */
#ifndef MPPI_AMD_AR_ROBUST_COST_HPP_
#define MPPI_AMD_AR_ROBUST_COST_HPP_

#include "mppi_amd/cost_functions/autorally/ar_standard_cost.hpp"

/** ar_robust_cost.cuh:6-29: ARStandardCostParams with the robust cost's defaults, and a trailing heading_coeff */
struct ARRobustCostParams : public ARStandardCostParams
{
  float heading_coeff = 0.0;

  ARRobustCostParams()
  {
    control_cost_coeff[0] = control_cost_coeff[1] = 0.0f;
    desired_speed = -1;  // -1: the speed map (channel .z) is the target
    boundary_threshold = 0.75;
    crash_coeff = 125000;
    max_slip_ang = 1.5;
    slip_coeff = 0.0;
    speed_coeff = 20.0;
    track_coeff = 33.0;
    track_slop = 0;
  }
};

template <class CLASS_T, class PARAMS_T = ARRobustCostParams>
class ARRobustCostImpl : public ARStandardCostImpl<CLASS_T, PARAMS_T>
{
public:
  using PARENT_CLASS = ARStandardCostImpl<CLASS_T, PARAMS_T>;
  /** the "costmap" blob of this class is {height, width, 4}: costmap_d_ points at interleaved texels */
  static constexpr int COSTMAP_CHANNELS = 4;

  /** one texel of the map; 16 bytes, loaded whole */
  struct alignas(16) Texel
  {
    float x, y, z, w;
  };

  ARRobustCostImpl(hipStream_t stream = 0) : PARENT_CLASS(stream)
  {
  }

  /** reference: ar_robust_cost.cu:13-37; the fp64 comparisons and ramp are the reference's (see the file comment) */
  __host__ __device__ inline float getStabilizingCost(const float* s) const
  {
    const PARAMS_T& p = this->params_;
    const bool standing = (double)fabsf(s[4]) < 0.001;
    const float slip = standing ? 0.0f : fabsf(-mppi::det::atan(s[5] / fabsf(s[4])));
    float charge = 0.0f;
    if ((double)slip >= 0.75 * (double)p.max_slip_ang)
    {
      // the ramp: 0 at three quarters of max_slip_ang, crash_coeff from max_slip_ang on
      const float share = fminf(1.0f, slip / p.max_slip_ang);
      charge = (float)(((double)share - 0.75) / (1.0 - 0.75)) * p.crash_coeff;
    }
    if ((double)fabsf(s[3]) >= 1.57079632679489661923)
      charge = p.crash_coeff;  // rolled over: instead of the ramp's charge, not on top of it
    return p.slip_coeff * slip + charge;
  }

  /** reference: ar_robust_cost.cu:39-112 (device branch) */
  __host__ __device__ inline float getCostmapCost(const float* s) const
  {
    const PARAMS_T& p = this->params_;
    float sin_yaw, cos_yaw;
    mppi::det::sincos(s[2], &sin_yaw, &cos_yaw);
    // both texel indices, then both loads, then the arithmetic: the loads are in flight together
    const int at_front = this->texelIndexTransformed(s[0] + this->FRONT_D * cos_yaw, s[1] + this->FRONT_D * sin_yaw);
    const int at_back = this->texelIndexTransformed(s[0] + this->BACK_D * cos_yaw, s[1] + this->BACK_D * sin_yaw);
    const Texel* map = reinterpret_cast<const Texel*>(this->costmap_d_);
    const Texel front = map[at_front];
    const Texel back = map[at_back];

    float total = 0;
    // boundary constraint of the worse end of the car: a ramp from boundary_threshold up to crash_coeff at 1
    const float boundary = fminf(1.0f, fmaxf(front.x, back.x));
    if (boundary >= p.boundary_threshold)
      total += (float)((double)(boundary - p.boundary_threshold) / (1.0 - (double)p.boundary_threshold)) * p.crash_coeff;
    // track position under the front of the car
    if (front.y > p.track_slop)
      total += p.track_coeff * front.y;
    // speed, L1: against the map's speed channel when desired_speed is -1
    const float target_speed = p.desired_speed == -1 ? front.z : p.desired_speed;
    total += p.speed_coeff * fabsf(s[4] - target_speed);
    // heading
    total += p.heading_coeff * fabsf(sin_yaw + front.w);
    return total;
  }

  /** reference: ar_robust_cost.cu:114-127; crash_status is not touched */
  __host__ __device__ inline float computeStateCost(const float* s, int timestep, float* theta_c, int* crash_status) const
  {
    const float total = getStabilizingCost(s) + getCostmapCost(s);
    const bool usable = total <= PARENT_CLASS::MAX_COST_VALUE;  // false for NaN too
    return usable ? total : PARENT_CLASS::MAX_COST_VALUE;
  }
};

class ARRobustCost : public ARRobustCostImpl<ARRobustCost>
{
public:
  /** no block barrier in the per-step device methods: may run on the role-separated kernels (plugin/parallel_utils.hpp) */
  static constexpr bool MPPI_BARRIER_FREE_STEP = true;
  /** a pure parameter block on the device (no device method stores to a member; the map pointer is a value read from the block,
   *  and the two texels are never the two arms of an address select): role loops may run it off the kernel's argument block */
  static constexpr bool MPPI_KERNARG_VIEWABLE = true;
  ARRobustCost(hipStream_t stream = 0) : ARRobustCostImpl<ARRobustCost>(stream)
  {
  }
};

#endif
