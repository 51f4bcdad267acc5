/**
 * QuadrotorMapCost plugin — the gate-racing cost of the quadrotor over a track map (reference:
 * include/mppi/cost_functions/quadrotor/quadrotor_map_cost.cuh:14-91 the parameters and their two host methods,
 * quadrotor_map_cost.cu:93-144 the DEVICE computeStateCost, :146-153 distToWaypoint, :199-395 the seven terms).
 *
 * The terms, each restated operation for operation and added in the reference's order (costmap, gate side, height, heading,
 * speed, attitude; then the gate reward; then the crash charge):
 *   computeCostmapCost      the track map under the vehicle, sampled through tex_helper_ (bilinear, fp32: the helper's own rule)
 *   computeGateSideCost     crash_coeff * |projection| when the vehicle is within min_dist_to_gate_side of the gate's line and
 *                           up to half a gate length beyond either post
 *   computeHeightCost       squared distance to a height interpolated between the previous and the current waypoint
 *   computeHeadingCost      the direction of flight against the bearing of the waypoint, outside gate_margin only
 *   computeSpeedCost        horizontal speed against desired_speed
 *   computeStabilizingCost  roll^2 + pitch^2
 *   computeWaypointCost     squared distance to the waypoint
 *
 * Quirks of the reference's device code that are KEPT:
 *   - waypoint_cost is computed and NOT added (quadrotor_map_cost.cu:105, :133); only the reference's host overload adds it
 *     (:74).  dist_to_waypoint_coeff therefore does nothing on the device, here as there.
 *   - crash_status is set when the gate term is non-zero, and `crash_status * crash_coeff` is added on that step and on EVERY
 *     later step of the rollout (:106-108, :142): the flag is the rollout's, nothing clears it.
 *   - leaving the map adds crash_coeff and STILL samples the (clamped) map, so the track terms are charged on top (:371-392).
 *   - `height_diff < 0` can never be true — height_diff is a square (:342-346); the branch is kept as written.
 *   - computeHeightCost mixes double constants into float arithmetic (`+ 0.001`, `1.0 - w1`, :338-340): the sums, the two
 *     divisions and the interpolation are evaluated in fp64 and rounded to float where the reference assigns to a float.
 *     Kept as written: eight fp64 operations per step.
 * What differs, on purpose:
 *   - transcendentals are mppi::det:: (atan2, sqrt; powf(a, p) is det::pow_pos(a, p) = exp(p log a), with powf's own values
 *     where exp(p log a) has none or need not be computed: a itself for p == 1, and 1 for p == 0 whatever a is — a heading
 *     error of exactly 0 would otherwise be exp(0 * -inf) = NaN);
 *   - the reference's device printf()s are dropped;
 *   - a NaN sum returns MAX_COST_VALUE, as QuadrotorQuadraticCost::nanToMaxCost does (the reference returns the NaN);
 *   - values the reference computes and never uses (the four distances to the gate posts, the left-hand projection,
 *     the vertical component of the world-frame velocity) are not computed;
 *   - the legacy CUDA-texture path (r_c1 / r_c2 / trs, coorTransform, queryTextureTransformed, loadTrackData), which the
 *     reference's device cost never reads, is not restated.  The three parameter fields stay, for layout.
 *
 * Order of evaluation (computeStateCost): straight-line, the map term first, as the reference has it.  The other order — the
 * map's footprint first, its four loads issued, the gate / height / heading / speed / attitude arithmetic, the interpolation last
 * — was built, gave the same bits, and measured 4 % SLOWER on the one-lane pipeline and 1.5 % slower on the fused kernel with nine
 * more VGPRs live across the arithmetic, so it is not kept ("Quadrotor map cost", has the figures).
 */
#ifndef MPPI_AMD_QUADROTOR_MAP_COST_HPP_
#define MPPI_AMD_QUADROTOR_MAP_COST_HPP_

#include <math.h>

#include "mppi_amd/plugin/cost.hpp"
#include "mppi_amd/dynamics/quadrotor/quadrotor_dynamics.hpp"
#include "mppi_amd/utils/texture_helpers/two_d_texture_helper.hpp"

/** quadrotor_map_cost.cuh:14-91; float3 / float4 as float[3] / float[4] so the block is a flat POD (model_params.h) */
struct QuadrotorMapCostParams : public CostParams<4>
{
  float r_c1[3] = { 1, 0, 0 };  ///< legacy texture transform, unused by the device cost (the reference leaves the three unset)
  float r_c2[3] = { 0, 1, 0 };
  float trs[3] = { 0, 0, 1 };

  float attitude_coeff = 10;
  float crash_coeff = 1000;
  float dist_to_waypoint_coeff = 0.0;
  float heading_coeff = 5;
  float heading_power = 1.0;  ///< power to take the difference in headings to
  float height_coeff = 5;
  float track_coeff = 10;
  float speed_coeff = 5;
  float track_slop = 0.0;
  float gate_pass_cost = -150;

  float curr_waypoint[4] = { 0, 0, 0, 0 };  ///< x, y, z, heading
  float prev_waypoint[4] = { 0, 0, 0, 0 };
  float curr_gate_left[3] = { 0, 0, 0 };
  float curr_gate_right[3] = { 0, 0, 0 };
  float prev_gate_left[3] = { 0, 0, 0 };
  float prev_gate_right[3] = { 0, 0, 0 };
  float end_waypoint[4] = { NAN, NAN, NAN, NAN };

  float desired_speed = 5;            ///< [m/s]
  float gate_margin = 0.5;            ///< [m]
  float min_dist_to_gate_side = 0.5;  ///< [m]
  float track_boundary_cost = 2.5;    ///< a costmap value above this is off the track
  float gate_width = 2.15;            ///< [m]

  QuadrotorMapCostParams()
  {
    for (int i = 0; i < 4; i++)
      this->control_cost_coeff[i] = 1;  // roll, pitch, yaw, throttle
  }

  /** quadrotor_map_cost.cuh:62-75: a new waypoint moves current to previous and places the gate's posts gate_width to either
   *  side of it along the heading (cosf / sinf on the host); the same waypoint again changes nothing.  Returns whether it changed. */
  bool updateWaypoint(float x, float y, float z, float heading = 0)
  {
    bool changed = false;
    if (curr_waypoint[0] != x || curr_waypoint[1] != y || curr_waypoint[2] != z || curr_waypoint[3] != heading)
    {
      for (int i = 0; i < 4; i++)
        prev_waypoint[i] = curr_waypoint[i];
      curr_waypoint[0] = x;
      curr_waypoint[1] = y;
      curr_waypoint[2] = z;
      curr_waypoint[3] = heading;
      updateGateBoundaries(x + cosf(heading) * gate_width, y + sinf(heading) * gate_width, z, x - cosf(heading) * gate_width,
                           y - sinf(heading) * gate_width, z);
      changed = true;
    }
    return changed;
  }

  /** quadrotor_map_cost.cuh:77-90 */
  bool updateGateBoundaries(float left_x, float left_y, float left_z, float right_x, float right_y, float right_z)
  {
    bool changed = false;
    if (curr_gate_left[0] != left_x || curr_gate_left[1] != left_y || curr_gate_left[2] != left_z || curr_gate_right[0] != right_x ||
        curr_gate_right[1] != right_y || curr_gate_right[2] != right_z)
    {
      for (int i = 0; i < 3; i++)
      {
        prev_gate_left[i] = curr_gate_left[i];
        prev_gate_right[i] = curr_gate_right[i];
      }
      curr_gate_left[0] = left_x;
      curr_gate_left[1] = left_y;
      curr_gate_left[2] = left_z;
      curr_gate_right[0] = right_x;
      curr_gate_right[1] = right_y;
      curr_gate_right[2] = right_z;
      changed = true;
    }
    return changed;
  }
};

class QuadrotorMapCost : public Cost<QuadrotorMapCost, QuadrotorMapCostParams, QuadrotorDynamicsParams>
{
public:
  using TexHelper = mppi::texture::TwoDTextureHelper<1, 1>;
  /** no block barrier in the per-step device methods: may run on the role-separated kernels (plugin/parallel_utils.hpp) */
  static constexpr bool MPPI_BARRIER_FREE_STEP = true;
  /** No device method stores to a member (the crash flag is the caller's), so a role loop may run the class off the kernel's
   *  argument block (engine/kernarg_view.hpp).  The object carries a device pointer, tex_helper_.textures_[0].data, as
   *  ARStandardCost carries costmap_d_: the pointer is a VALUE read from the block, and the map behind it is only ever loaded
   *  through it — border_color and the map are never the two arms of one select (see computeStateCost) — so the condition holds. */
  static constexpr bool MPPI_KERNARG_VIEWABLE = true;
  static constexpr float MAX_COST_VALUE = 1e16;

  /** the track map: one texture, one channel; the engine fills it from the "costmap" / "costmap_transform" blobs
   *  (engine/model_blobs.hpp: bindMap, setMapFrame).  Not in use (checkTextureUse(0) false) means the map term is 0. */
  TexHelper tex_helper_;

  QuadrotorMapCost(hipStream_t stream = nullptr)
  {
    bindToStream(stream);
  }

  /** quadrotor_map_cost.cu:156-196: the parameter methods on the object; true when something changed (the caller's
   *  setCostParams / the templated controller's next computeControl carries it to the engine) */
  bool updateWaypoint(float x, float y, float z, float heading = 0)
  {
    const bool changed = this->params_.updateWaypoint(x, y, z, heading);
    if (changed)
      (void)paramsToDevice();
    return changed;
  }
  bool updateGateBoundaries(float left_x, float left_y, float left_z, float right_x, float right_y, float right_z)
  {
    const bool changed = this->params_.updateGateBoundaries(left_x, left_y, left_z, right_x, right_y, right_z);
    if (changed)
      (void)paramsToDevice();
    return changed;
  }

  /** MAX_COST_VALUE for a NaN (see the note at the top of the file) */
  __host__ __device__ static inline float nanToMaxCost(float cost)
  {
    return (cost != cost) ? MAX_COST_VALUE : cost;
  }

  /** quadrotor_map_cost.cu:146-153 */
  __host__ __device__ inline float distToWaypoint(const float* s, const float* waypoint) const
  {
    return mppi::det::sqrt(SQ(s[E_INDEX(OutputIndex, POS_X)] - waypoint[0]) + SQ(s[E_INDEX(OutputIndex, POS_Y)] - waypoint[1]) +
                           SQ(s[E_INDEX(OutputIndex, POS_Z)] - waypoint[2]));
  }

  /** quadrotor_map_cost.cu:199-208 */
  __host__ __device__ inline float computeStabilizingCost(const float* s) const
  {
    float cost = 0;
    float roll, pitch, yaw;
    mppi::math::Quat2EulerNWU(&s[E_INDEX(OutputIndex, QUAT_W)], roll, pitch, yaw);
    const float quat_dist_from_level = SQ(roll) + SQ(pitch);
    cost += this->params_.attitude_coeff * quat_dist_from_level;
    return cost;
  }

  /** quadrotor_map_cost.cu:210-238: yaw is the direction of R v, the state's velocity turned by the attitude */
  __host__ __device__ inline float computeHeadingCost(const float* s) const
  {
    const QuadrotorMapCostParams& p = this->params_;
    float cost = 0;
    float R[3][3];
    mppi::math::Quat2DCM(&s[E_INDEX(OutputIndex, QUAT_W)], R);
    const float vx = s[E_INDEX(OutputIndex, VEL_X)], vy = s[E_INDEX(OutputIndex, VEL_Y)], vz = s[E_INDEX(OutputIndex, VEL_Z)];
    const float w_v_x = R[0][0] * vx + R[0][1] * vy + R[0][2] * vz;
    const float w_v_y = R[1][0] * vx + R[1][1] * vy + R[1][2] * vz;
    const float yaw = mppi::det::atan2(w_v_y, w_v_x);

    // heading to the gate
    const float wx = p.curr_waypoint[0] - s[E_INDEX(OutputIndex, POS_X)];
    const float wy = p.curr_waypoint[1] - s[E_INDEX(OutputIndex, POS_Y)];
    const float w_heading = mppi::det::atan2(wy, wx);

    const float dist_to_gate = distToWaypoint(s, p.curr_waypoint);
    // far away from the gate the vehicle should fly towards it
    if (dist_to_gate > p.gate_margin)
    {
      const float a = fabsf(angle_utils::shortestAngularDistance(w_heading, yaw));
      cost += p.heading_coeff * headingPow(a, p.heading_power);
    }
    return cost;
  }
  /** powf(a, power) for a >= 0 (see the note at the top of the file) */
  __host__ __device__ static inline float headingPow(float a, float power)
  {
    return power == 1.0f ? a : (power == 0.0f ? 1.0f : mppi::det::pow_pos(a, power));
  }

  /** quadrotor_map_cost.cu:240-253 */
  __host__ __device__ inline float computeSpeedCost(const float* s) const
  {
    const float speed = mppi::det::sqrt(s[E_INDEX(OutputIndex, VEL_X)] * s[E_INDEX(OutputIndex, VEL_X)] +
                                        s[E_INDEX(OutputIndex, VEL_Y)] * s[E_INDEX(OutputIndex, VEL_Y)]);
    return this->params_.speed_coeff * SQ(speed - this->params_.desired_speed);
  }

  /** quadrotor_map_cost.cu:255-262 */
  __host__ __device__ inline float computeWaypointCost(const float* s) const
  {
    const float dist_to_gate = distToWaypoint(s, this->params_.curr_waypoint);
    return this->params_.dist_to_waypoint_coeff * SQ(dist_to_gate);
  }

  /**
   * quadrotor_map_cost.cu:264-323.  gate_vec runs from the right post to the left one; perp_dist is the cross product of the
   * vehicle's offset from the right post with it (NOT divided by the gate's length, as there); the projection is 0 at the
   * right post and 1 at the left one.  A hit: |perp_dist| < min_dist_to_gate_side and the projection in [-0.5, 0) or (1, 1.5].
   */
  __host__ __device__ inline float computeGateSideCost(const float* s) const
  {
    const QuadrotorMapCostParams& p = this->params_;
    float cost = 0;
    const float gate_x = p.curr_gate_left[0] - p.curr_gate_right[0], gate_y = p.curr_gate_left[1] - p.curr_gate_right[1];
    const float right_x = s[E_INDEX(OutputIndex, POS_X)] - p.curr_gate_right[0];
    const float right_y = s[E_INDEX(OutputIndex, POS_Y)] - p.curr_gate_right[1];
    const float perp_dist = right_x * gate_y - right_y * gate_x;
    const float comp_state_along_gate_right = (right_x * gate_x + right_y * gate_y) / (gate_x * gate_x + gate_y * gate_y);
    const float threshold = 0.5;
    if (fabsf(perp_dist) < p.min_dist_to_gate_side &&
        ((comp_state_along_gate_right < 0.0f && comp_state_along_gate_right >= 0.0f - threshold) ||
         (comp_state_along_gate_right > 1.0f && comp_state_along_gate_right <= 1.0f + threshold)))
    {
      cost += p.crash_coeff * fabsf(comp_state_along_gate_right);
    }
    return cost;
  }

  /** quadrotor_map_cost.cu:325-357; the double constants and what they promote are kept (see the top of the file) */
  __host__ __device__ inline float computeHeightCost(const float* s) const
  {
    const QuadrotorMapCostParams& p = this->params_;
    float cost = 0;
    const float d1 = mppi::det::sqrt(SQ(s[E_INDEX(OutputIndex, POS_X)] - p.prev_waypoint[0]) +
                                     SQ(s[E_INDEX(OutputIndex, POS_Y)] - p.prev_waypoint[1]));
    const float d2 = mppi::det::sqrt(SQ(s[E_INDEX(OutputIndex, POS_X)] - p.curr_waypoint[0]) +
                                     SQ(s[E_INDEX(OutputIndex, POS_Y)] - p.curr_waypoint[1]));

    const float w1 = d1 / (d1 + d2 + 0.001);
    const float w2 = d2 / (d1 + d2 + 0.001);
    const float interpolated_height = (1.0 - w1) * p.prev_waypoint[2] + (1.0 - w2) * p.curr_waypoint[2];

    const float height_diff = SQ(fabsf(s[E_INDEX(OutputIndex, POS_Z)] - interpolated_height));
    if (height_diff < 0)
    {
      cost += p.crash_coeff * (1 - height_diff);
    }
    else
    {
      cost += p.height_coeff * height_diff;
    }
    if (height_diff > p.gate_width)
    {
      cost += 400;
    }
    return cost;
  }

  /** quadrotor_map_cost.cu:359-395.  The lookup is the helper's queryTexture: it forms the interpolated value first and chooses
   *  the border colour against it afterwards — two VALUES, never the addresses of the map and of this object
   *  (two_d_texture_helper.hpp) */
  __host__ __device__ inline float computeCostmapCost(const float* s) const
  {
    const QuadrotorMapCostParams& p = this->params_;
    float cost = 0;
    if (!tex_helper_.checkTextureUse(0))
    {
      return cost;
    }
    const float query_point[3] = { s[E_INDEX(OutputIndex, POS_X)], s[E_INDEX(OutputIndex, POS_Y)], s[E_INDEX(OutputIndex, POS_Z)] };
    float map_pose[3], tex_coords[3];
    tex_helper_.worldPoseToMapPose(0, query_point, map_pose);
    tex_helper_.mapPoseToTexCoord(0, map_pose, tex_coords);
    if (tex_coords[0] < 0.0f || tex_coords[0] > 1.0f || tex_coords[1] < 0.0f || tex_coords[1] > 1.0f)
    {  // the vehicle is not in the map anymore
      cost += p.crash_coeff;
    }
    float track_cost;
    tex_helper_.queryTexture(0, tex_coords, &track_cost);
    // cost from the distance to the centre line of the track
    if (track_cost > p.track_slop)
    {
      cost += p.track_coeff * track_cost;
    }
    if (track_cost > p.track_boundary_cost)
    {  // the costmap says this point is no longer on the track
      cost += p.crash_coeff;
    }
    return cost;
  }

  /** quadrotor_map_cost.cu:93-144 */
  __host__ __device__ inline float computeStateCost(float* s, int timestep = 0, float* theta_c = nullptr, int* crash_status = nullptr)
  {
    float cost = 0;
    float costmap_cost, gate_cost, height_cost, heading_cost, speed_cost, stable_cost;
    float waypoint_cost;
    costmap_cost = computeCostmapCost(s);
    gate_cost = computeGateSideCost(s);
    height_cost = computeHeightCost(s);
    heading_cost = computeHeadingCost(s);
    speed_cost = computeSpeedCost(s);
    stable_cost = computeStabilizingCost(s);
    waypoint_cost = computeWaypointCost(s);
    (void)waypoint_cost;  // computed, not added: see the top of the file
    if (gate_cost != 0)
    {
      *crash_status = 1;
    }

    cost += costmap_cost + gate_cost + height_cost + heading_cost + speed_cost + stable_cost;

    // decrease the cost when passing the gate
    const float dist_to_gate = distToWaypoint(s, this->params_.curr_waypoint);
    if (dist_to_gate < this->params_.gate_margin)
    {
      cost += this->params_.gate_pass_cost;
    }
    cost += *crash_status * this->params_.crash_coeff;
    return nanToMaxCost(cost);
  }

  /** quadrotor_map_cost.cu:403-407 */
  __host__ __device__ inline float terminalCost(float* s, float* theta_c = nullptr)
  {
    return 0;
  }
};

#endif
