/**
 * QuadrotorVolumeCost plugin — QuadrotorQuadraticCost plus a clearance volume.  NOT in the reference: it exists so that the 3-D
 * texture helper (utils/texture_helpers/three_d_texture_helper.hpp) runs, is tested and is measured where a plugin would use it,
 * inside the rollout kernels.
 *
 *   cost(s) = quadratic(s) + volume_coeff * max(0, v) + (v > crash_threshold ? crash_coeff : 0)
 *
 * quadratic(s) is QuadrotorQuadraticCost::computeStateCost with the same parameters, in the same order of additions (its NaN guard
 * included: a NaN sum is MAX_COST_VALUE before the volume terms are added).  v is channel 0 of a one-channel volume sampled at the
 * vehicle's world position with queryTextureAtWorldPose — think of an occupancy or inverse-clearance field, 0 in free space and
 * rising towards obstacles.  The volume's three axes address in BORDER mode with border colour 0 by default: outside the mapped
 * volume the term is 0.  Without the "cost_volume" blob (checkTextureUse(0) false) the term is 0 everywhere.
 *
 * The crash term is a per-step charge; it does not set the rollout's crash flag.  terminalCost is the quadratic cost's:
 * terminal_cost_coeff times the quadratic part, without the volume.
 */
#ifndef MPPI_AMD_QUADROTOR_VOLUME_COST_HPP_
#define MPPI_AMD_QUADROTOR_VOLUME_COST_HPP_

#include <math.h>

#include "mppi_amd/plugin/cost.hpp"
#include "mppi_amd/cost_functions/quadrotor/quadrotor_quadratic_cost.hpp"
#include "mppi_amd/dynamics/quadrotor/quadrotor_dynamics.hpp"
#include "mppi_amd/utils/texture_helpers/three_d_texture_helper.hpp"

/** QuadrotorQuadraticCostParams and the volume term's three numbers; a flat POD (mppi_quadrotor_volume_cost_params) */
struct QuadrotorVolumeCostParams : public QuadrotorQuadraticCostParams
{
  float volume_coeff = 10.0f;
  float crash_threshold = 0.9f;
  float crash_coeff = 1000.0f;
};

class QuadrotorVolumeCost : public Cost<QuadrotorVolumeCost, QuadrotorVolumeCostParams, QuadrotorDynamicsParams>
{
public:
  using VolumeHelper = mppi::texture::ThreeDTextureHelper<1, 1>;
  /** no block barrier in the per-step device methods: may run on the role-separated kernels (plugin/parallel_utils.hpp) */
  static constexpr bool MPPI_BARRIER_FREE_STEP = true;
  /** No device method stores to a member, so a role loop may run the class off the kernel's argument block
   *  (engine/kernarg_view.hpp).  The object carries a device pointer, volume_helper_.textures_[0].data; the volume behind it is
   *  only ever loaded through it, and the border colour is chosen against the interpolated VALUE (three_d_texture_helper.hpp). */
  static constexpr bool MPPI_KERNARG_VIEWABLE = true;
  static constexpr float MAX_COST_VALUE = 1e16;

  /** the clearance volume: one texture, one channel; the engine fills it from the "cost_volume" / "cost_volume_transform" blobs
   *  (engine/model_blobs.hpp: bindVolume, setMapFrame) */
  VolumeHelper volume_helper_;

  QuadrotorVolumeCost(hipStream_t stream = nullptr)
  {
    for (int axis = 0; axis < 3; axis++)
      volume_helper_.textures_[0].address_mode[axis] = mppi::texture::ADDRESS_BORDER;
    bindToStream(stream);
  }

  __host__ __device__ static inline float nanToMaxCost(float cost)
  {
    return (cost != cost) ? MAX_COST_VALUE : cost;
  }

  /** QuadrotorQuadraticCost::computeStateCost (quadrotor_quadratic_cost.hpp), statement for statement, on this class's parameters */
  __host__ __device__ inline float quadraticCost(const float* s) const
  {
    const QuadrotorVolumeCostParams& p = this->params_;
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
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
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

  /** v: the volume's value at the vehicle's position; 0 without a volume */
  __host__ __device__ inline float volumeValue(const float* s) const
  {
    if (!volume_helper_.checkTextureUse(0))
      return 0.0f;
    const float position[3] = { s[E_INDEX(OutputIndex, POS_X)], s[E_INDEX(OutputIndex, POS_Y)], s[E_INDEX(OutputIndex, POS_Z)] };
    float v;
    volume_helper_.queryTextureAtWorldPose(0, position, &v);
    return v;
  }

  /** volume_coeff * max(0, v) + (v > crash_threshold ? crash_coeff : 0) */
  __host__ __device__ inline float volumeCost(const float v) const
  {
    const QuadrotorVolumeCostParams& p = this->params_;
    float cost = p.volume_coeff * fmaxf(0.0f, v);
    if (v > p.crash_threshold)
      cost += p.crash_coeff;
    return cost;
  }

  __host__ __device__ inline float computeStateCost(float* s, int timestep = 0, float* theta_c = nullptr, int* crash_status = nullptr)
  {
    // the lookup first: its eight loads are in flight under the quaternion arithmetic of the quadratic part
    const float v = volumeValue(s);
    const float quadratic = quadraticCost(s);
    return nanToMaxCost(quadratic + volumeCost(v));
  }

  __host__ __device__ inline float terminalCost(float* s, float* theta_c = nullptr)
  {
    return nanToMaxCost(this->params_.terminal_cost_coeff * quadraticCost(s));
  }
};

#endif
