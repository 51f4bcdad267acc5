/**
 * model_instance.hpp — type-erased wrapper around one (DYN, COST, SAMPLER) template instantiation.
 *
 * The C ABI cannot carry templates, so each registered model is one ModelT<...> object behind the ModelBase
 * interface — the role played in the reference by its explicit instantiations
 * (reference: include/mppi/instantiations/cartpole_mppi/cartpole_mppi.cuh, src/controllers/cartpole/cartpole_mppi.cu:30-42).
 * Block shapes are compile-time (see rollout_kernel.hpp); each model lists the shapes it is instantiated for.
 *
 * The pieces around ModelT: model_base.hpp (ModelBase and the ABI fingerprint), model_traits.hpp (what a plugin class has),
 * model_launch.hpp (the one checked launch path), model_blobs.hpp (the bulk-data checks and uploads).
 */
#ifndef MPPI_AMD_MODEL_INSTANCE_HPP_
#define MPPI_AMD_MODEL_INSTANCE_HPP_

#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "mppi_amd.h"
#include "hip_owned.hpp"
#include "kernarg_view.hpp"
#include "model_base.hpp"
#include "model_traits.hpp"
#include "model_launch.hpp"
#include "model_blobs.hpp"
#include "rollout_kernel.hpp"
#include "finalize_kernel.hpp"
#include "rollout_pipeline_kernel.hpp"
#include "rmppi_kernels.hpp"
#include "rmppi_pipeline_kernel.hpp"
#include "linearize_kernel.hpp"
#include "mppi_amd/feedback_controllers/ddp_feedback.hpp"
#include "mppi_amd/sampling_distributions/colored_noise.hpp"

namespace mppi
{
namespace engine
{
template <class DYN_T, int BY>
__global__ void __launch_bounds__(BY) modelStepKernel(DYN_T dynamics_obj, float* x_d, float* u_d, float dt, int enforce)
{
  MPPI_ASSUME_BLOCK_SHAPE(1, BY, 1);
  DYN_T* dynamics = &dynamics_obj;
  constexpr int S = DYN_T::STATE_DIM, C = DYN_T::CONTROL_DIM, O = DYN_T::OUTPUT_DIM;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* theta_s = reinterpret_cast<float*>(smem_raw);
  float* x = theta_s + calcClassSharedMemSize(dynamics, 1) / (int)sizeof(float);
  float* xn = x + math::nearest_multiple_4(S);
  float* xdot = xn + math::nearest_multiple_4(S);
  float* u = xdot + math::nearest_multiple_4(S);
  float* y = u + math::nearest_multiple_4(C);
  const int ty = (int)__builtin_amdgcn_workitem_id_y();
  for (int i = ty; i < S; i += BY)
  {
    x[i] = x_d[i];
    xdot[i] = 0.0f;
  }
  for (int i = ty; i < C; i += BY)
    u[i] = u_d[i];
  for (int i = ty; i < O; i += BY)
    y[i] = 0.0f;
  __syncthreads();
  dynamics->initializeDynamics(x, u, y, theta_s, 0.0f, dt);
  __syncthreads();
  if (enforce)
  {
    dynamics->enforceConstraints(x, u);
    __syncthreads();
  }
  dynamics->step(x, xn, xdot, u, y, theta_s, 0, dt);
  __syncthreads();
  for (int i = ty; i < S; i += BY)
    x_d[i] = xn[i];
  for (int i = ty; i < C; i += BY)
    u_d[i] = u[i];
}

}  // namespace engine
namespace kernels
{
/** the block's sample rows exactly as the rollout kernels see them after initializeDistributions(): raw eps[k][t][c]
 *  (pre-filled modes only), block = 64 rollouts x one lane */
template <class SAMPLING_T>
__global__ void __launch_bounds__(64) noiseDumpKernel(SAMPLING_T sampling_obj, float* out_d)
{
  SAMPLING_T* sampling = &sampling_obj;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* theta_d = reinterpret_cast<float*>(smem_raw);
  sampling->initializeDistributions(nullptr, 0.0f, 0.0f, theta_d);
  __syncthreads();
  const int T = sampling->params_.num_timesteps;
  const int TC = T * SAMPLING_T::CONTROL_DIM;
  const int stride = SAMPLING_T::rowStride(T);
  const int row0 = (int)blockIdx.x * 64;
  const int nrows = min(64, sampling->params_.num_rollouts - row0);
  for (int e = (int)threadIdx.x; e < nrows * TC; e += 64)
  {
    const int r = e / TC, j = e - r * TC;
    out_d[(size_t)(row0 + r) * TC + j] = theta_d[r * stride + j];
  }
}
}  // namespace kernels
namespace engine
{
/**
 * DYN_FAST_T / FAST_SHAPES: an optional second Dynamics type implementing the same model for particular block shapes
 * (e.g. the MFMA forward of the NN model for shape (16, 4)); it is constructed from the primary object at launch, so
 * parameters, control ranges and blobs are shared.
 */
template <class DYN_T, class COST_T, class SAMPLING_T, class SHAPES, int FIN_BY = 1, class DYN_FAST_T = void,
          class FAST_SHAPES = Shapes<>, bool PIPELINE = false, bool RMPPI = false>
struct ModelT : ModelBase
{
  /* ---- Robust MPPI: block = (64 rollouts, 1, 2 systems), one lane per rollout and system ---- */
  DeviceDDP<DYN_T> fb;
  HipBuffer<float> gains_d;
  bool supportsRMPPI() const override
  {
    return RMPPI;
  }
  mppi_status setFeedbackGains(const float* gains, int T, bool accumulate_all_states, bool gains_on_device, hipStream_t stream,
                               std::string& err) override
  {
    if constexpr (RMPPI)
    {
      const size_t n = (size_t)T * DYN_T::STATE_DIM * DYN_T::CONTROL_DIM;
      hipError_t e = hipSuccess;
      if (gains_d.size() != n)
      {
        e = hipStreamSynchronize(stream);  // earlier launches may still read the old gains
        if (e == hipSuccess)
          e = gains_d.alloc(n);
      }
      if (e == hipSuccess)
        e = hipMemcpyAsync(gains_d, gains, n * sizeof(float), gains_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream);
      if (e == hipSuccess)
        e = hipStreamSynchronize(stream);
      fb.fb_gain_traj_d_ = gains_d;  // null after a failed allocation, never a freed buffer
      if (e != hipSuccess)
      {
        err = std::string("feedback gain upload: ") + hipGetErrorString(e);
        return MPPI_ERR_HIP;
      }
      fb.num_timesteps_ = T;
      fb.accumulate_all_states_ = accumulate_all_states;
      return MPPI_OK;
    }
    return ModelBase::setFeedbackGains(gains, T, accumulate_all_states, gains_on_device, stream, err);
  }
  /* ---- the forms of a model: the object a kernel takes.  The model itself (`dyn`); its replicated-lane form REP_T(dyn) (MFMA /
   *  four-lane dynamics); the form that class may name for ONE rollout on a wave, REP_T::FINALIZE_FORM(dyn) (NN models: lane =
   *  neuron, utils/nn_helpers/fnn_wave.hpp); and the form it may name for the role-pipelined Robust kernels, RMPPI_PIPE_T(dyn)
   *  (`using RMPPI_PIPELINE_FORM = ...` — a class of the same arithmetic whose trade-offs are made for a block of 11-15 waves at
   *  128-168 VGPRs each: dynamics/racer_dubins/racer_dubins_elevation_lstm_unc.hpp).  A form is built from `dyn` at the launch, so
   *  parameters, control ranges and blobs are shared. ---- */
  using REP_T = DYN_FAST_T;
  static constexpr bool HAS_REP = !std::is_void<REP_T>::value;
  static constexpr bool HAS_WAVE = has_finalize_form<REP_T>::value;
  template <class T, class = void>
  struct rmppi_pipeline_form
  {
    using type = T;
  };
  template <class T>
  struct rmppi_pipeline_form<T, std::void_t<typename T::RMPPI_PIPELINE_FORM>>
  {
    using type = typename T::RMPPI_PIPELINE_FORM;
  };
  using RMPPI_PIPE_T = std::conditional_t<HAS_REP, typename rmppi_pipeline_form<REP_T>::type, DYN_T>;
  /** the four-lane forms of the RACER models are compiled for the reference's network shapes: a model that says which networks it
   *  holds (`register_form_`) has a replicated-lane form for some of them only, every other one for whatever is loaded */
  static constexpr bool REP_ALWAYS = HAS_REP && !has_register_form<DYN_T>::value;
  /** can the replicated-lane form take the networks loaded now */
  bool repUsable() const
  {
    if constexpr (HAS_REP && !REP_ALWAYS)
      return dyn.register_form_;
    else
      return HAS_REP;
  }
  /** f(form): FORM_T built from the model, or the model itself */
  template <class FORM_T, class F>
  auto withForm(F&& f)
  {
    if constexpr (std::is_same<FORM_T, DYN_T>::value)
      return f(dyn);
    else
    {
      FORM_T form(dyn);
      return f(form);
    }
  }
  /** Robust MPPI's fused kernels run on the replicated-lane form of a model when it is usable, else on the model itself, one lane
   *  per rollout and system (round 3; a network of another shape used to be refused).  f(rm_dyn): the object the kernels take. */
  template <class F>
  auto withRmppiDynamics(F&& f)
  {
    if constexpr (!REP_ALWAYS)
    {
      if (!repUsable())
        return f(dyn);
    }
    return withForm<std::conditional_t<HAS_REP, REP_T, DYN_T>>(f);
  }

  /** this launch draws its noise inside the step loop: the sampler can, and no noise was injected */
  bool drawsInLoop() const
  {
    return SAMPLING_T::IN_LOOP_DRAW && smp.noise_source_ == 0;
  }
  /** the instantiation of a kernel template this launch takes, over DRAW_IN_LOOP x ROWS_HBM: k(draw, hbm) names one, the two given
   *  as std::bool_constant values.  HBM_FORMS: the template has forms for the sample rows in HBM (long horizons) — instantiated for
   *  samplers that support them only; DRAW: this block shape can draw in the loop. */
  template <bool HBM_FORMS, bool DRAW = SAMPLING_T::IN_LOOP_DRAW, class K>
  auto kernelVariant(K k) const
  {
    constexpr std::bool_constant<DRAW> draw{};
    constexpr std::false_type no{};
    const bool in_loop = DRAW && drawsInLoop();
    auto kfn = in_loop ? k(draw, no) : k(no, no);
    if constexpr (HBM_FORMS && SAMPLING_T::SUPPORTS_GLOBAL_ROWS)
    {
      if (smp.rows_global_d_)
        kfn = in_loop ? k(draw, std::true_type{}) : k(no, std::true_type{});
    }
    return kfn;
  }
  /** the one writer of last_launch: a rollout launch that went out leaves what it ran */
  mppi_status noted(mppi_status st, int family, int bx, int by, int bz, bool streamed_merge)
  {
    if (st == MPPI_OK)
      last_launch = LaunchRecord{family, bx, by, bz, smp.rows_global_d_ != nullptr, streamed_merge};
    return st;
  }

  /* ---- Robust MPPI: one function per launch family gives its block (LDS bytes, threads, rings); the LDS queries and the
   *  launches both read it ---- */
  template <class RM_DYN_T>
  BlockPlan<> rmppiPlan(const RM_DYN_T& rm_dyn, int bx) const
  {
    return {kernels::rmppiSharedBytes(rm_dyn, cost, fb, smp, bx), dim3(bx * kernels::replicated_lanes<RM_DYN_T>::value, 1, 2), bx, 0};
  }
  /** smem 0: not even the shortest rings fit next to the sample rows */
  template <class PD_T>
  BlockPlan<kernels::RMPPIPipeRings> rmppiPipelinePlan(const PD_T& pd) const
  {
    const kernels::RMPPIPipeRings r = kernels::rmppiPipelineRings(pd, cost, fb, smp, MAX_LDS_BYTES);
    return {r.out_steps ? kernels::rmppiPipelineSharedBytes(pd, cost, fb, smp, r) : 0,
            dim3(64 * kernels::rmppiPipelineWaves<PD_T>(), 1, 1), 64, r};
  }
  template <class RM_DYN_T>
  BlockPlan<> initEvalPlan(const RM_DYN_T& rm_dyn) const
  {
    return {kernels::initEvalSharedBytes<RM_DYN_T, COST_T, SAMPLING_T>(rm_dyn, cost, 64),
            dim3(64 * kernels::replicated_lanes<RM_DYN_T>::value, 1, 1), 64, 0};
  }
  /** ring 0: the rows of 64 rollouts and a ring do not fit the LDS */
  template <class PD_T>
  BlockPlan<> initEvalPipelinePlan(const PD_T& pd, int T) const
  {
    const int ring = kernels::initEvalPipelineRing(pd, cost, T, MAX_LDS_BYTES);
    constexpr int WAVES = kernels::replicated_lanes<PD_T>::value + kernels::INIT_EVAL_PIPE_SAMPLERS + kernels::INIT_EVAL_PIPE_COSTS;
    return {ring ? kernels::initEvalPipelineSharedBytes(pd, cost, T, ring) : 0, dim3(64 * WAVES, 1, 1), 64, ring};
  }
  size_t rmppiSharedBytes(int bx, int T) override
  {
    if constexpr (RMPPI)
    {
      smp.params_.num_timesteps = T;
      smp.params_.num_distributions = 2;
      return withRmppiDynamics([&](auto& rm_dyn) { return rmppiPlan(rm_dyn, bx).smem; });
    }
    return 0;
  }
  /** the role-pipelined Robust MPPI kernels (rmppi_pipeline_kernel.hpp) exist for models with a replicated-lane form, and for
   *  models registered for the role-pipelined rollout (PIPELINE: one lane per rollout, no block barrier inside the per-step
   *  methods) — with a sampler whose rows may live in HBM and need no block-wide prologue of their own (the Gaussian one) */
  static constexpr bool rmppiHasPipeline()
  {
    if constexpr (!RMPPI || !SAMPLING_T::SUPPORTS_GLOBAL_ROWS || SAMPLING_T::COLORED)
      return false;
    else if constexpr (HAS_REP)
      return kernels::replicated_lanes<REP_T>::value > 1;
    else
      return PIPELINE;
  }
  /** can the pipelined kernels run with the networks loaded right now (replicated-lane forms exist for one shape only) */
  bool rmppiPipelineUsable() const
  {
    return rmppiHasPipeline() && (!HAS_REP || repUsable());
  }
  size_t rmppiPipelineSharedBytes(int T) override
  {
    if constexpr (rmppiHasPipeline())
    {
      if (!rmppiPipelineUsable())
        return 0;
      smp.params_.num_timesteps = T;
      smp.params_.num_distributions = 2;
      return withForm<RMPPI_PIPE_T>([&](auto& pd) { return rmppiPipelinePlan(pd).smem; });
    }
    return 0;
  }
  mppi_status launchRMPPIPipeline(const kernels::RMPPIArgs& a, hipStream_t stream, std::string& err)
  {
    if constexpr (rmppiHasPipeline())
    {
      return withForm<RMPPI_PIPE_T>([&](auto& pd) -> mppi_status {
        using PD_T = std::decay_t<decltype(pd)>;
        const auto p = rmppiPipelinePlan(pd);
        if (p.ring.out_steps == 0)
          return refuse(MPPI_ERR_LDS_OVERFLOW,
                        "pipelined RMPPI rollout kernel: the rings do not fit 160 KiB of LDS next to the sample rows", err);
        auto kfn = kernelVariant<false>([](auto draw, auto) {
          return kernels::rolloutRMPPIPipelineKernel<PD_T, COST_T, DeviceDDP<DYN_T>, SAMPLING_T, decltype(draw)::value>;
        });
        return launchChecked("rolloutRMPPIPipelineKernel", kfn, p.grid(a.base.num_rollouts), p.block, p.smem, stream, err, pd, cost,
                             fb, smp, a, p.ring);
      });
    }
    return refuse(MPPI_ERR_LAUNCH_SHAPE, "model has no role-pipelined Robust MPPI kernel", err);
  }
  mppi_status launchInitEval(bool pipeline, const kernels::InitEvalArgs& a, const SamplerLaunchState& s, hipStream_t stream,
                             std::string& err) override
  {
    if constexpr (RMPPI)
    {
      if (!blobsReady(err))
        return MPPI_ERR_STATE;
      prepSampler(s);
      if constexpr (rmppiHasPipeline())
      {
        // the candidate rollouts as blocks of role waves (rmppi_pipeline_kernel.hpp) when the rows of 64 rollouts and a ring
        // fit the LDS; else the fused kernel below
        if (pipeline && rmppiPipelineUsable())
        {
          bool launched = false;
          const mppi_status st = withForm<RMPPI_PIPE_T>([&](auto& pd) -> mppi_status {
            const BlockPlan<> p = initEvalPipelinePlan(pd, a.num_timesteps);
            if (p.ring == 0)
              return MPPI_OK;
            launched = true;
            return launchChecked("initEvalPipelineKernel", kernels::initEvalPipelineKernel<std::decay_t<decltype(pd)>, COST_T, SAMPLING_T>,
                                 p.grid(a.num_eval_rollouts), p.block, p.smem, stream, err, pd, cost, smp, a, p.ring);
          });
          if (launched || st != MPPI_OK)
            return st;
        }
      }
      return withRmppiDynamics([&](auto& rm_dyn) -> mppi_status {
        const BlockPlan<> p = initEvalPlan(rm_dyn);
        return launchChecked("initEvalKernel", kernels::initEvalKernel<std::decay_t<decltype(rm_dyn)>, COST_T, SAMPLING_T, 64>,
                             p.grid(a.num_eval_rollouts), p.block, p.smem, stream, err, rm_dyn, cost, smp, a);
      });
    }
    return ModelBase::launchInitEval(pipeline, a, s, stream, err);
  }
  template <int BX>
  mppi_status launchRMPPIShape(const kernels::RMPPIArgs& a, hipStream_t stream, std::string& err)
  {
    if constexpr (RMPPI)
    {
      return withRmppiDynamics([&](auto& rm_dyn) -> mppi_status {
        using RM_DYN_T = std::decay_t<decltype(rm_dyn)>;
        const BlockPlan<> p = rmppiPlan(rm_dyn, BX);
        if (p.smem > MAX_LDS_BYTES)
          return ldsOverflow("RMPPI rollout kernel", p.smem, err);
        auto kfn = kernelVariant<false>([](auto draw, auto) {
          return kernels::rolloutRMPPIKernel<RM_DYN_T, COST_T, DeviceDDP<DYN_T>, SAMPLING_T, BX, decltype(draw)::value>;
        });
        return launchChecked("rolloutRMPPIKernel", kfn, p.grid(a.base.num_rollouts), p.block, p.smem, stream, err, rm_dyn, cost, fb,
                             smp, a);
      });
    }
    return refuse(MPPI_ERR_UNSUPPORTED, "model is not registered for Robust MPPI", err);
  }
  /** the family of a Robust rollout launch, in order of precedence; MPPI_FAMILY_NONE: no kernel for such a block.  32 rollouts: for
   *  horizons whose sample rows for 64 rollouts x 2 systems do not fit the LDS */
  int rmppiFamily(int bx, bool pipeline) const
  {
    if (pipeline && bx == 64 && rmppiPipelineUsable())
      return MPPI_FAMILY_RMPPI_PIPELINE;
    return bx == 64 || bx == 32 ? MPPI_FAMILY_RMPPI : MPPI_FAMILY_NONE;
  }
  mppi_status launchRMPPI(int bx, bool pipeline, const kernels::RMPPIArgs& a, const SamplerLaunchState& s, hipStream_t stream,
                          std::string& err) override
  {
    if constexpr (RMPPI)
    {
      if (!blobsReady(err))
        return MPPI_ERR_STATE;
      if (!fb.fb_gain_traj_d_ || fb.num_timesteps_ != s.num_timesteps)
        return refuse(MPPI_ERR_STATE,
                      "Robust MPPI needs the DDP feedback gains [T][S][C] (mppi_set_feedback_gains) before it can run", err);
      prepSampler(s);
      const int family = rmppiFamily(bx, pipeline);
      if (family == MPPI_FAMILY_NONE)
        return refuse(MPPI_ERR_LAUNCH_SHAPE, "Robust MPPI rollout kernel is instantiated for 64 or 32 rollouts per block", err);
      return noted(family == MPPI_FAMILY_RMPPI_PIPELINE ? launchRMPPIPipeline(a, stream, err) :
                   bx == 64                             ? launchRMPPIShape<64>(a, stream, err) :
                                                          launchRMPPIShape<32>(a, stream, err),
                   family, bx, 1, 2, false);
    }
    return ModelBase::launchRMPPI(bx, pipeline, a, s, stream, err);
  }

  bool supportsPipeline() const override
  {
    return PIPELINE;
  }
  bool supportsRMPPIPipeline() const override
  {
    return rmppiHasPipeline();
  }
  /** does the instantiation ask for role-separated kernels (the one-lane pipeline, or the replicated-lane one), and do the
   *  classes those kernels would run say that their per-step methods hold no block barrier? */
  static constexpr bool ROLE_SEPARATED = PIPELINE || HAS_REP;
  static constexpr bool fastDeclared()
  {
    if constexpr (!HAS_REP)
      return true;
    else
      return mppi::barrier_free_step<REP_T>::value;
  }
  static constexpr bool BARRIER_FREE_DECLARED = (!PIPELINE || mppi::barrier_free_step<DYN_T>::value) && fastDeclared() &&
                                                (!ROLE_SEPARATED || (mppi::barrier_free_step<COST_T>::value &&
                                                                     mppi::barrier_free_step<SAMPLING_T>::value));
  std::string undeclaredBarrierFreePlugins() const override
  {
    std::string missing;
    if constexpr (ROLE_SEPARATED)
    {
      if (PIPELINE && !mppi::barrier_free_step<DYN_T>::value)
        missing += "Dynamics ";
      if (!fastDeclared())
        missing += "Dynamics(replicated-lane form) ";
      if (!mppi::barrier_free_step<COST_T>::value)
        missing += "Cost ";
      if (!mppi::barrier_free_step<SAMPLING_T>::value)
        missing += "SamplingDistribution ";
    }
    return missing;
  }
  bool supportsStreamedMerge() const override
  {
    return PIPELINE && SAMPLING_T::IN_LOOP_DRAW && !SAMPLING_T::COLORED;
  }
  bool supportsPipelineRep(int bx, int by, int bz) const override
  {
    if constexpr (HAS_REP)
      return bx == 64 && bz == 1 && by == kernels::replicated_lanes<REP_T>::value && hasShape(FAST_SHAPES{}, bx, by, bz);
    return false;
  }
  bool fastShapeRefused(int bx, int by, int bz) const override
  {
    return HAS_REP && !repUsable() && hasShape(FAST_SHAPES{}, bx, by, bz);
  }
  bool supportsPipelineFold(int bx, int by, int bz) const override
  {
    return PIPELINE && bx == 32 && by == 1 && bz == 2;
  }

  DYN_T dyn;
  COST_T cost;
  SAMPLING_T smp;
  /* colored noise: basis table cache */
  HipBuffer<float> basis_d;
  int basis_T = -1, basis_stride = -1;
  bool basis_dirty = true;
  HipBuffer<float> weights_d;
  HipBuffer<float> weights2_d;
  static_assert(!(has_costmap<COST_T>::value && has_cost_texture<COST_T>::value),
                "a cost class takes its map as costmap_d_ or through a tex_helper_, not both");
  HipBuffer<float> costmap_d;
  HipBuffer<float> cost_volume_d;
  HipBuffer<float> elevation_d;
  HipBuffer<float> normals_d;
  bool normals_transform_set = false;
  HipBuffer<float> extra_net_d[4];  ///< mean LSTM, mean MLP, uncertainty LSTM, uncertainty MLP

  /** the checks, uploads and bindings are model_blobs.hpp's; here: which blob names a model has, and where each one goes */
  mppi_status setBlob(const std::string& name, const float* data, size_t count, const int* dims, int ndims,
                      hipStream_t stream, std::string& err) override
  {
    if constexpr (has_fnn_helper<DYN_T>::value)
    {
      if (name == "dynamics_weights")
      {
        if (!expectCount(name, count, dyn.helper_.NUM_PARAMS, err))
          return MPPI_ERR_INVALID_ARG;
        const mppi_status st = uploadBlob(weights_d, data, count, stream, err);
        dyn.helper_.theta_d_ = weights_d;
        return st;
      }
    }
    if constexpr (has_lstm_structure<DYN_T>::value)
    {
      /* the reference sizes its LSTM from the network file (LSTMHelper(npz), lstm_helper.cu:13-62); here the shape is
       * {hidden size, output-network layer sizes ...} as floats, given before the weights */
      if (name == "lstm_structure")
      {
        const std::vector<int> desc(data, data + count);
        if (!dyn.setLSTMStructure(desc.data(), (int)count))
        {
          err = "lstm_structure: expected {H, H + inputs, ..., outputs} with at least one output-network layer";
          return MPPI_ERR_INVALID_ARG;
        }
        dyn.lstm_.weights_d_ = nullptr;  // blobs of the previous shape no longer fit
        dyn.lstm_.output_nn_.theta_d_ = nullptr;
        return MPPI_OK;
      }
    }
    if constexpr (has_lstm_helper<DYN_T>::value)
    {
      if (name == "lstm_weights")
      {
        if (!expectCount(name, count, dyn.lstm_.getNumParams(), err))
          return MPPI_ERR_INVALID_ARG;
        const mppi_status st = uploadBlob(weights_d, data, count, stream, err);
        dyn.lstm_.weights_d_ = weights_d;
        return st;
      }
      if (name == "lstm_output_weights")
      {
        if (!expectCount(name, count, dyn.lstm_.output_nn_.NUM_PARAMS, err))
          return MPPI_ERR_INVALID_ARG;
        const mppi_status st = uploadBlob(weights2_d, data, count, stream, err);
        dyn.lstm_.output_nn_.theta_d_ = weights2_d;
        return st;
      }
    }
    if constexpr (has_elevation_map<DYN_T>::value)
    {
      /* {height, width} heights, row-major */
      if (name == "elevation_map")
      {
        if (!checkMapDims(name, dims, ndims, count, 1, err))
          return MPPI_ERR_INVALID_ARG;
        const mppi_status st = uploadBlob(elevation_d, data, count, stream, err);
        bindMap(dyn.tex_helper_.textures_[0], elevation_d, dims, st);
        return st;
      }
      if (name == "elevation_map_transform")
      {
        if (!expectFrameCount(name, count, err))
          return MPPI_ERR_INVALID_ARG;
        setMapFrame(dyn.tex_helper_.textures_[0], data);
        if constexpr (has_normals_map<DYN_T>::value)
        {  // the normals map shares the frame unless it was given its own
          if (!normals_transform_set)
            setMapFrame(dyn.normals_tex_helper_.textures_[0], data);
        }
        return MPPI_OK;
      }
    }
    if constexpr (has_mean_unc_networks<DYN_T>::value)
    {
      /* LSTMLSTMHelper(path, "terra/mean_network/") / (…, "terra/uncertainty_network/") (racer_dubins_elevation_lstm_unc.cu:30-33):
       * parameter blobs in the layouts of lstm_helper.hpp / fnn_helper.hpp; "<net>_lstm_state" = [hidden | cell], the
       * per-cycle update of updateFromBuffer (:98-141), written in place */
      if (name == "mean_lstm_structure" || name == "unc_lstm_structure")
      {
        /* another hidden size / output network than the reference's test shapes: {H, H + inputs, ..., outputs} as floats,
         * given before the weights (the reference sizes the networks from the file, lstm_helper.cu:13-62) */
        const int which = name[0] == 'm' ? 1 : 2;
        const std::vector<int> desc(data, data + count);
        if (!dyn.setNetworkStructure(which, desc.data(), (int)count))
        {
          err = name + ": expected {H, H + inputs, ..., outputs} with the model's input / output sizes (12 -> 2, 13 -> 5)";
          return MPPI_ERR_INVALID_ARG;
        }
        // blobs of the previous shape no longer fit
        for (int k = 2 * (which - 1); k < 2 * which; k++)
          extra_net_d[k].reset();
        (which == 1 ? dyn.mean_lstm_d_ : dyn.unc_lstm_d_) = nullptr;
        (which == 1 ? dyn.mean_fnn_d_ : dyn.unc_fnn_d_) = nullptr;
        (which == 1 ? dyn.mean_lstm_ : dyn.unc_lstm_).weights_d_ = nullptr;
        (which == 1 ? dyn.mean_lstm_ : dyn.unc_lstm_).output_nn_.theta_d_ = nullptr;
        return MPPI_OK;
      }
      const struct
      {
        const char* name;
        int slot;
        size_t count;
      } nets[6] = { { "mean_lstm_weights", 0, (size_t)dyn.mean_lstm_.getNumParams() },
                    { "mean_lstm_output_weights", 1, (size_t)dyn.mean_lstm_.output_nn_.NUM_PARAMS },
                    { "unc_lstm_weights", 2, (size_t)dyn.unc_lstm_.getNumParams() },
                    { "unc_lstm_output_weights", 3, (size_t)dyn.unc_lstm_.output_nn_.NUM_PARAMS },
                    { "mean_lstm_state", 0, (size_t)2 * dyn.mean_lstm_.HIDDEN_DIM },
                    { "unc_lstm_state", 2, (size_t)2 * dyn.unc_lstm_.HIDDEN_DIM } };
      for (int i = 0; i < 6; i++)
      {
        if (name != nets[i].name)
          continue;
        if (!expectCount(name, count, nets[i].count, err))
          return MPPI_ERR_INVALID_ARG;
        if (i >= 4)
        {  // initial hidden / cell state into the tail of the uploaded LSTM blob
          float* blob = extra_net_d[nets[i].slot];
          if (!blob)
          {
            err = "set the network's weights before its state";
            return MPPI_ERR_STATE;
          }
          const size_t params = (size_t)(i == 4 ? dyn.mean_lstm_.LSTM_NUM_PARAMS : dyn.unc_lstm_.LSTM_NUM_PARAMS);
          return uploadTail(blob, params, data, count, "LSTM state upload", stream, err);
        }
        const mppi_status st = uploadBlob(extra_net_d[nets[i].slot], data, count, stream, err);
        // only what was uploaded for the present shapes (a structure blob clears its network's pair)
        if (nets[i].slot == 0)
          dyn.mean_lstm_.weights_d_ = dyn.mean_lstm_d_ = extra_net_d[0];
        else if (nets[i].slot == 1)
          dyn.mean_lstm_.output_nn_.theta_d_ = dyn.mean_fnn_d_ = extra_net_d[1];
        else if (nets[i].slot == 2)
          dyn.unc_lstm_.weights_d_ = dyn.unc_lstm_d_ = extra_net_d[2];
        else
          dyn.unc_lstm_.output_nn_.theta_d_ = dyn.unc_fnn_d_ = extra_net_d[3];
        return st;
      }
    }
    if constexpr (has_normals_map<DYN_T>::value)
    {
      /* getTextureHelperNormals()->updateTexture(0, float4 data) (racer_dubins_elevation_suspension_lstm.cuh:131-134; the tests'
       * set-up tests/dynamics/racer_dubins_elevation_suspension_test.cu:170-190): {height, width, 4} = nx, ny, nz, unused */
      if (name == "normals_map")
      {
        if (!checkMapDims(name, dims, ndims, count, 4, err))
          return MPPI_ERR_INVALID_ARG;
        const mppi_status st = uploadBlob(normals_d, data, count, stream, err);
        bindMap(dyn.normals_tex_helper_.textures_[0], normals_d, dims, st);
        return st;
      }
      if (name == "normals_map_transform")
      {
        if (!expectFrameCount(name, count, err))
          return MPPI_ERR_INVALID_ARG;
        setMapFrame(dyn.normals_tex_helper_.textures_[0], data);
        normals_transform_set = true;
        return MPPI_OK;
      }
    }
    if constexpr (has_costmap<COST_T>::value)
    {
      if (name == "costmap")
      {
        /* CH > 1: interleaved texels, one CH-float texel per map cell (ARRobustCost: boundary, track position, speed, heading) */
        constexpr int CH = costmap_channels<COST_T>::value;
        if (!checkMapDims(name, dims, ndims, count, CH, err))
        {
          if constexpr (CH > 1)
            err = "costmap: this model's cost reads " + std::to_string(CH) + " channels: dims must be {height, width, " +
                  std::to_string(CH) + "} (interleaved texels) with height*width*" + std::to_string(CH) + " == count";
          return MPPI_ERR_INVALID_ARG;
        }
        const mppi_status st = uploadBlob(costmap_d, data, count, stream, err);
        cost.costmap_d_ = costmap_d;
        cost.height_ = dims[0];
        cost.width_ = dims[1];
        return st;
      }
    }
    if constexpr (has_cost_texture<COST_T>::value)
    {
      /* the cost's TwoDTextureHelper: {height, width} values, row-major; the model runs without it */
      if (name == "costmap")
      {
        if (!checkMapDims(name, dims, ndims, count, 1, err))
          return MPPI_ERR_INVALID_ARG;
        const mppi_status st = uploadBlob(costmap_d, data, count, stream, err);
        bindMap(cost.tex_helper_.textures_[0], costmap_d, dims, st);
        return st;
      }
      if (name == "costmap_transform")
      {
        if (!expectFrameCount(name, count, err))
          return MPPI_ERR_INVALID_ARG;
        setMapFrame(cost.tex_helper_.textures_[0], data);
        return MPPI_OK;
      }
    }
    if constexpr (has_cost_volume<COST_T>::value)
    {
      /* the cost's ThreeDTextureHelper: {depth, height, width} values, row-major layers; the model runs without it */
      if (name == "cost_volume")
      {
        if (!checkMapDims(name, dims, ndims, count, std::remove_reference_t<decltype(cost.volume_helper_)>::CHANNELS, err, 3))
          return MPPI_ERR_INVALID_ARG;
        const mppi_status st = uploadBlob(cost_volume_d, data, count, stream, err);
        bindVolume(cost.volume_helper_.textures_[0], cost_volume_d, dims, st);
        return st;
      }
      if (name == "cost_volume_transform")
      {
        if (!expectFrameCount(name, count, err))
          return MPPI_ERR_INVALID_ARG;
        setMapFrame(cost.volume_helper_.textures_[0], data);
        return MPPI_OK;
      }
    }
    return ModelBase::setBlob(name, data, count, dims, ndims, stream, err);
  }

  mppi_status setLSTMInitialState(const float* hidden, const float* cell, hipStream_t stream, std::string& err) override
  {
    if constexpr (has_lstm_helper<DYN_T>::value)
    {
      if (!weights_d || !dyn.lstm_.weights_d_)
      {
        err = "set the 'lstm_weights' blob before the initial hidden / cell state";
        return MPPI_ERR_STATE;
      }
      const int H = dyn.lstm_.HIDDEN_DIM;
      std::vector<float> state(2 * (size_t)H);  // [hidden | cell], the layout behind the blob's parameters
      for (int i = 0; i < H; i++)
      {
        if (!std::isfinite(hidden[i]) || !std::isfinite(cell[i]))
        {  // det::tanh(NaN) = -1: a NaN recurrent state would be masked, not propagated (see mppi_set_model_blob)
          err = "non-finite hidden / cell state";
          return MPPI_ERR_NAN;
        }
        state[i] = hidden[i];
        state[H + i] = cell[i];
      }
      return uploadTail(weights_d, dyn.lstm_.LSTM_NUM_PARAMS, state.data(), state.size(), "LSTM initial state upload", stream, err);
    }
    return ModelBase::setLSTMInitialState(hidden, cell, stream, err);
  }

  int costmapChannels() const override
  {
    if constexpr (has_costmap<COST_T>::value)
      return costmap_channels<COST_T>::value;
    return 0;
  }
  mppi_status setCostmapTransform(const float* r_c1, const float* r_c2, const float* trs) override
  {
    if constexpr (has_costmap<COST_T>::value)
    {
      for (int i = 0; i < 3; i++)
      {
        cost.params_.r_c1[i] = r_c1[i];
        cost.params_.r_c2[i] = r_c2[i];
        cost.params_.trs[i] = trs[i];
      }
      return MPPI_OK;
    }
    return MPPI_ERR_INVALID_ARG;
  }

  /** models with bulk data must have it before the first launch */
  bool blobsReady(std::string& err) const
  {
    if constexpr (has_fnn_helper<DYN_T>::value)
      if (!dyn.helper_.theta_d_)
      {
        err = "model needs the 'dynamics_weights' blob (mppi_set_model_blob) before it can run";
        return false;
      }
    if constexpr (has_lstm_helper<DYN_T>::value)
      if (!dyn.lstm_.weights_d_ || !dyn.lstm_.output_nn_.theta_d_)
      {
        err = "model needs the 'lstm_weights' and 'lstm_output_weights' blobs (mppi_set_model_blob) before it can run";
        return false;
      }
    if constexpr (has_costmap<COST_T>::value)
      if (!cost.costmap_d_)
      {
        err = "model needs the 'costmap' blob (mppi_set_model_blob) before it can run";
        return false;
      }
    if constexpr (has_mean_unc_networks<DYN_T>::value)
      if (!dyn.mean_lstm_d_ || !dyn.mean_fnn_d_ || !dyn.unc_lstm_d_ || !dyn.unc_fnn_d_)
      {
        err = "model needs the 'mean_lstm_weights', 'mean_lstm_output_weights', 'unc_lstm_weights' and "
              "'unc_lstm_output_weights' blobs (mppi_set_model_blob) before it can run";
        return false;
      }
    return true;
  }

  ModelT()
  {
    S = DYN_T::STATE_DIM;
    C = DYN_T::CONTROL_DIM;
    O = DYN_T::OUTPUT_DIM;
  }

  mppi_status setDynamicsParams(const void* pod, size_t n) override
  {
    // the params struct adds its fields after the (empty) DynamicsParams base: a flat block of floats / ints
    if (std::is_empty<typename DYN_T::DYN_PARAMS_T>::value)
      return n == 0 ? MPPI_OK : MPPI_ERR_INVALID_ARG;
    if (n != sizeof(typename DYN_T::DYN_PARAMS_T))
      return MPPI_ERR_INVALID_ARG;
    memcpy((void*)&dyn.params_, pod, n);
    return MPPI_OK;
  }
  mppi_status setCostParams(const void* pod, size_t n) override
  {
    if (n != sizeof(typename COST_T::COST_PARAMS_T))
      return MPPI_ERR_INVALID_ARG;
    memcpy((void*)&cost.params_, pod, n);
    return MPPI_OK;
  }
  void setControlRanges(const float* lo_hi) override
  {
    for (int i = 0; i < DYN_T::CONTROL_DIM; i++)
    {
      dyn.control_rngs_[i].x = lo_hi[2 * i];
      dyn.control_rngs_[i].y = lo_hi[2 * i + 1];
    }
  }
  void setControlDeadband(const float* db) override
  {
    for (int i = 0; i < DYN_T::CONTROL_DIM; i++)
      dyn.control_deadband_[i] = db[i];
  }
  void getZeroControl(float* out) const override
  {
    for (int i = 0; i < DYN_T::CONTROL_DIM; i++)
      out[i] = dyn.zero_control_[i];
  }
  void hostEnforceLeash(const float* state_true, const float* state_nominal, const float* leash, float* out) const override
  {
    if constexpr (has_host_leash<DYN_T>::value)
      dyn.enforceLeash(state_true, state_nominal, leash, out);
    else
      ModelBase::hostEnforceLeash(state_true, state_nominal, leash, out);
  }
  bool hostEnforceConstraints(float* u) const override
  {
    if (!DYN_T::BASE_CONSTRAINTS || DYN_T::CONSTRAINTS_DEPEND_ON_STATE)
      return false;
    for (int i = 0; i < DYN_T::CONTROL_DIM; i++)
    {  // the operations of Dynamics::enforceConstraints (plugin/dynamics.hpp), correctly rounded on either side
      if (fabsf(u[i]) < dyn.control_deadband_[i])
        u[i] = dyn.zero_control_[i];
      else
        u[i] += dyn.control_deadband_[i] * -mppi::math::sign(u[i]);
      u[i] = fminf(fmaxf(dyn.control_rngs_[i].x, u[i]), dyn.control_rngs_[i].y);
    }
    return true;
  }
  void setSamplerParams(const mppi_gaussian_params* p, int D) override
  {
    for (int i = 0; i < DYN_T::CONTROL_DIM * D && i < DYN_T::CONTROL_DIM * 2; i++)
      smp.params_.std_dev[i] = p->std_dev[i];
    if (D == 1)  // keep distribution 1 defined (copyStdDevToDistribution semantics, gaussian.cuh:45-60)
      for (int i = 0; i < DYN_T::CONTROL_DIM; i++)
        smp.params_.std_dev[DYN_T::CONTROL_DIM + i] = p->std_dev[i];
    for (int i = 0; i < DYN_T::CONTROL_DIM; i++)
      smp.params_.control_cost_coeff[i] = p->control_cost_coeff[i];
    smp.params_.pure_noise_trajectories_percentage = p->pure_noise_trajectories_percentage;
    smp.params_.std_dev_decay = p->std_dev_decay;
    smp.params_.sum_strides = p->sum_strides;
  }

  void setTimeSpecificStdDev(const float* table_d) override
  {
    smp.std_dev_time_d_ = table_d;
    smp.params_.time_specific_std_dev = table_d != nullptr;
  }
  mppi_status setColoredNoiseParams(const float* exponents, float offset_decay_rate, float fmin) override
  {
    if constexpr (SAMPLING_T::COLORED)
    {
      for (int i = 0; i < DYN_T::CONTROL_DIM; i++)
        smp.exponents_[i] = exponents[i];
      smp.offset_decay_rate_ = offset_decay_rate;
      smp.fmin_ = fmin;
      basis_dirty = true;
      return MPPI_OK;
    }
    return MPPI_ERR_STATE;
  }
  size_t noiseFloatsPerRollout(int T) const override
  {
    if constexpr (SAMPLING_T::COLORED)
      return (size_t)DYN_T::CONTROL_DIM * sampling_distributions::coloredSpectrumFloats(T);
    return (size_t)DYN_T::CONTROL_DIM * T;
  }
  /** colored noise: (re)build the basis table for this (T, optimization_stride, parameters) and upload it */
  mppi_status prepBasis(const SamplerLaunchState& s, hipStream_t stream, std::string& err)
  {
    if constexpr (SAMPLING_T::COLORED)
    {
      if (basis_dirty || basis_T != s.num_timesteps || basis_stride != s.optimization_stride)
      {
        std::vector<float> frag;
        const bool radix4 = sampling_distributions::coloredUseRadix4(s.num_timesteps, s.optimization_stride);
        if (radix4)  // T a multiple of 4: two FFT decimation steps in front of a GEMM a quarter the size (colored_noise.hpp)
          sampling_distributions::buildColoredNoiseBasisRadix4(s.num_timesteps, DYN_T::CONTROL_DIM, smp.exponents_,
                                                               smp.offset_decay_rate_, smp.fmin_, frag);
        else
          sampling_distributions::buildColoredNoiseBasis(s.num_timesteps, DYN_T::CONTROL_DIM, smp.exponents_,
                                                         smp.offset_decay_rate_, smp.fmin_, s.optimization_stride, frag);
        hipError_t e = hipStreamSynchronize(stream);  // earlier launches may still read the old table
        if (e == hipSuccess && (!basis_d || basis_T != s.num_timesteps || basis_d.size() != frag.size()))
          e = basis_d.alloc(frag.size());
        if (e == hipSuccess)
          e = hipMemcpyAsync(basis_d, frag.data(), frag.size() * sizeof(float), hipMemcpyHostToDevice, stream);
        if (e == hipSuccess)
          e = hipStreamSynchronize(stream);  // frag is a local
        smp.basis_d_ = basis_d;  // null after a failed allocation, never a freed buffer
        if (e != hipSuccess)
        {
          err = std::string("colored-noise basis upload: ") + hipGetErrorString(e);
          return MPPI_ERR_HIP;
        }
        basis_T = s.num_timesteps;
        basis_stride = s.optimization_stride;
        basis_dirty = false;
      }
      smp.basis_d_ = basis_d;
    }
    return MPPI_OK;
  }

  mppi_status launchNoiseDump(const SamplerLaunchState& s, float* out_d, hipStream_t stream, std::string& err) override
  {
    if (SAMPLING_T::IN_LOOP_DRAW && !s.eps_d)
      return refuse(MPPI_ERR_UNSUPPORTED, "noise dump: this sampler draws inside the step loop; use mppi_philox_normal for its stream", err);
    prepSampler(s);
    mppi_status st = prepBasis(s, stream, err);
    if (st != MPPI_OK)
      return st;
    smp.params_.num_distributions = 1;
    SAMPLING_T dump_smp = smp;
    dump_smp.rows_global_d_ = nullptr;  // the dump kernel reads the rows back from ITS LDS, whatever the rollouts use
    const size_t smem = calcClassSharedMemSize(&dump_smp, 64);
    if (smem > MAX_LDS_BYTES)
      return refuse(MPPI_ERR_LDS_OVERFLOW, "noise dump kernel: the rows of 64 rollouts do not fit the LDS at this horizon", err);
    return launchChecked("noiseDumpKernel", kernels::noiseDumpKernel<SAMPLING_T>, dim3((s.num_rollouts_local + 63) / 64),
                         dim3(64, 1, 1), smem, stream, err, dump_smp, out_d);
  }

  template <class LIST>
  static bool hasShape(LIST list, int bx, int by, int bz)
  {
    return forShape(list, bx, by, bz, [](auto) {});
  }
  bool supportsShape(int bx, int by, int bz) const override
  {
    return hasShape(SHAPES{}, bx, by, bz) || hasShape(FAST_SHAPES{}, bx, by, bz);
  }
  template <class LIST>
  static void appendShapes(LIST list, std::vector<int>& out)
  {
    anyShape(list, [&](auto s) {
      out.insert(out.end(), {s.x, s.y, s.z});
      return false;
    });
  }
  void listShapes(std::vector<int>& out) const override
  {
    appendShapes(FAST_SHAPES{}, out);  // the MFMA shapes first: preferred at equal rollouts per block
    appendShapes(SHAPES{}, out);
  }
  void listReplicatedLaneShapes(std::vector<int>& out) const override
  {
    appendShapes(FAST_SHAPES{}, out);
  }

  void prepSampler(const SamplerLaunchState& s)
  {
    smp.params_.num_rollouts = s.num_rollouts_local;
    smp.params_.num_timesteps = s.num_timesteps;
    smp.params_.num_distributions = s.num_distributions;
    smp.control_means_d_ = s.control_means_d;
    smp.eps_d_ = s.eps_d;
    smp.control_samples_d_ = s.control_samples_d;
    smp.noise_source_ = s.eps_d ? 1 /* NOISE_EPS_BUFFER */ : 0 /* NOISE_PHILOX_FUSED */;
    smp.seed_ = s.seed;
    smp.generation_ = s.generation;
    smp.rollout_offset_ = s.rollout_offset;
    smp.num_rollouts_global_ = s.num_rollouts_global;
    smp.params_.use_same_noise_for_all_distributions = s.independent_noise == 0;
    smp.setIteration(s.iteration, s.optimization_stride);
  }

  size_t globalRowsFloats(int blocks, int slots, int T) const override
  {
    if constexpr (SAMPLING_T::SUPPORTS_GLOBAL_ROWS)
      return (size_t)blocks * slots * SAMPLING_T::rowStrideGlobal(T);
    return 0;
  }
  void setGlobalRows(float* rows_d) override
  {
    if constexpr (SAMPLING_T::SUPPORTS_GLOBAL_ROWS)
      smp.rows_global_d_ = rows_d;
  }

  /* ---- the rollout launch: one decision of the family, one function per family for its block; rolloutSharedBytes (what
   *  planLaunch decides on) and launchRollout both go through them ---- */
  /** the family of a rollout launch, in order of precedence; MPPI_FAMILY_NONE: the shape is not instantiated */
  int rolloutFamily(int bx, int by, int bz, bool pipeline) const
  {
    if (pipeline)
      return ModelT::supportsPipelineRep(bx, by, bz)  ? MPPI_FAMILY_PIPELINE_REP :
             ModelT::supportsPipelineFold(bx, by, bz) ? MPPI_FAMILY_PIPELINE_FOLD :
                                                        MPPI_FAMILY_PIPELINE;
    if (HAS_REP && hasShape(FAST_SHAPES{}, bx, by, bz))
      return MPPI_FAMILY_FUSED_REP;
    return hasShape(SHAPES{}, bx, by, bz) ? MPPI_FAMILY_FUSED : MPPI_FAMILY_NONE;
  }
  /** ring 0, MAX_LDS_BYTES + 1 bytes: the sample rows leave no room for the output ring */
  template <class FAST>
  BlockPlan<> pipelineRepPlan(const FAST& fast) const
  {
    const int ring = kernels::pipelineRepRingSteps(fast, cost, smp, MAX_LDS_BYTES);
    constexpr int WAVES = kernels::replicated_lanes<FAST>::value + kernels::PIPE_REP_SAMPLERS + kernels::PIPE_REP_COSTS;
    return {ring ? kernels::pipelineRepSharedBytes(fast, cost, smp, ring) : MAX_LDS_BYTES + 1, dim3(64 * WAVES, 1, 1), 64, ring};
  }
  BlockPlan<> pipelinePlan(int z, bool fold) const
  {
    return {kernels::pipelineSharedBytes(dyn, cost, smp, z, fold), dim3(kernels::pipelineBlockX(z, fold), 1, fold ? 1 : z),
            fold ? 64 / z : 64, 0};
  }
  /** rolloutKernel on one form: `by` contract lanes, each rollout on replicated_lanes<FORM_T> lanes of x */
  template <class FORM_T>
  BlockPlan<> fusedPlan(const FORM_T& form, int bx, int by, int bz) const
  {
    return {kernels::rolloutSharedBytes(form, cost, smp, bx, by, bz), dim3(bx * kernels::replicated_lanes<FORM_T>::value, by, bz), bx, 0};
  }
  size_t rolloutSharedBytes(int bx, int by, int bz, int T, int D, bool pipeline) override
  {
    smp.params_.num_timesteps = T;
    smp.params_.num_distributions = D;
    const int family = rolloutFamily(bx, by, bz, pipeline);
    if constexpr (HAS_REP)
    {
      if (family == MPPI_FAMILY_PIPELINE_REP || family == MPPI_FAMILY_FUSED_REP)
      {
        REP_T rep(dyn);
        return family == MPPI_FAMILY_PIPELINE_REP ? pipelineRepPlan(rep).smem : fusedPlan(rep, bx, 1, bz).smem;
      }
    }
    return pipeline ? pipelinePlan(bz, family == MPPI_FAMILY_PIPELINE_FOLD).smem : fusedPlan(dyn, bx, by, bz).smem;
  }

  template <class FAST = REP_T>
  mppi_status launchPipelineRep(const kernels::RolloutArgs& args, hipStream_t stream, std::string& err)
  {
    if constexpr (!std::is_void<FAST>::value)
    {
      FAST fast(dyn);
      const BlockPlan<> p = pipelineRepPlan(fast);
      if (p.ring == 0)
        return refuse(MPPI_ERR_LDS_OVERFLOW,
                      "pipeline rollout kernel: the sample rows leave no room for the output ring in 160 KiB of LDS", err);
      auto kfn = kernelVariant<true>([](auto draw, auto hbm) {
        return kernels::rolloutPipelineRepKernel<FAST, COST_T, SAMPLING_T, decltype(draw)::value, decltype(hbm)::value>;
      });
      return launchChecked("rolloutPipelineRepKernel", kfn, p.grid(args.num_rollouts), p.block, p.smem, stream, err, fast, cost, smp,
                           args, p.ring);
    }
    return refuse(MPPI_ERR_LAUNCH_SHAPE, "model has no replicated-lane dynamics", err);
  }
  template <int Z, bool FOLD = false>
  mppi_status launchPipeline(const kernels::RolloutArgs& args, hipStream_t stream, std::string& err)
  {
    if constexpr (PIPELINE)
    {
      const BlockPlan<> p = pipelinePlan(Z, FOLD);
      if (p.smem > MAX_LDS_BYTES)
        return ldsOverflow("pipeline rollout kernel", p.smem, err);
      auto kfn = kernelVariant<true>([](auto draw, auto hbm) {
        return kernels::rolloutPipelineKernel<DYN_T, COST_T, SAMPLING_T, Z, decltype(draw)::value, FOLD, decltype(hbm)::value>;
      });
      if constexpr (Z == 1 && !FOLD && SAMPLING_T::IN_LOOP_DRAW && !SAMPLING_T::COLORED)
      {
        // the previous iteration's block records merged by this launch's sampler waves (RolloutArgs::prev_records_d)
        if (args.prev_records_d && args.prev_records_t_d && drawsInLoop() && !smp.rows_global_d_)
          kfn = kernels::rolloutPipelineKernel<DYN_T, COST_T, SAMPLING_T, 1, SAMPLING_T::IN_LOOP_DRAW, false, false, true>;
        else if (args.prev_records_d)
          return refuse(MPPI_ERR_STATE,
                        "prev_records_d: this launch cannot merge the previous records itself (noise source / rows in HBM / no "
                        "transposed copy)",
                        err);
      }
      else if (args.prev_records_d)
        return refuse(MPPI_ERR_STATE, "prev_records_d: the streamed merge exists for one-system Gaussian pipeline launches only", err);
      return launchChecked("rolloutPipelineKernel", kfn, p.grid(args.num_rollouts), p.block, p.smem, stream, err, dyn, cost, smp, args);
    }
    return refuse(MPPI_ERR_LAUNCH_SHAPE, "model is not registered for the pipeline variant", err);
  }
  /** rolloutKernel for one registered shape on `form`.  The replicated-lane form runs shape (X, REP, Z) as X rollouts x REP
   *  replicated lanes with one contract lane (BY = 1).  The in-loop Philox draw needs one lane per rollout; otherwise the rows are
   *  pre-filled by initializeDistributions. */
  template <class SHAPE, class FORM_T>
  mppi_status launchFused(SHAPE, FORM_T& form, const kernels::RolloutArgs& args, hipStream_t stream, std::string& err)
  {
    constexpr bool OWN = std::is_same<FORM_T, DYN_T>::value;
    constexpr int X = SHAPE::x, BY = OWN ? SHAPE::y : 1, Z = SHAPE::z;
    static_assert(OWN || kernels::replicated_lanes<FORM_T>::value == SHAPE::y, "fast shape: BY must equal the plugin's REPLICATED_LANES");
    const BlockPlan<> p = fusedPlan(form, X, BY, Z);
    if (p.smem > MAX_LDS_BYTES)
      return ldsOverflow("rollout kernel", p.smem, err);
    auto kfn = kernelVariant<false, (BY == 1) && SAMPLING_T::IN_LOOP_DRAW>([](auto draw, auto) {
      return kernels::rolloutKernel<FORM_T, COST_T, SAMPLING_T, X, BY, Z, decltype(draw)::value>;
    });
    return launchChecked(OWN ? "rolloutKernel" : "rolloutKernel (fast variant)", kfn, p.grid(args.num_rollouts), p.block, p.smem, stream,
                         err, form, cost, smp, args);
  }
  mppi_status launchRollout(int bx, int by, int bz, bool pipeline, const kernels::RolloutArgs& args,
                            const SamplerLaunchState& s, hipStream_t stream, std::string& err) override
  {
    if (!blobsReady(err))
      return MPPI_ERR_STATE;
    prepSampler(s);
    mppi_status st = prepBasis(s, stream, err);
    if (st != MPPI_OK)
      return st;
    if (ModelT::fastShapeRefused(bx, by, bz))
      return refuse(MPPI_ERR_LAUNCH_SHAPE,
                    "the replicated-lane block shapes of this model exist for its default network shape only: create the "
                    "controller with block_y = 1 for a network set through 'lstm_structure'",
                    err);
    const int family = rolloutFamily(bx, by, bz, pipeline);
    switch (family)
    {
      case MPPI_FAMILY_PIPELINE_REP:
        st = launchPipelineRep(args, stream, err);
        break;
      case MPPI_FAMILY_PIPELINE_FOLD:
        st = launchPipeline<2, true>(args, stream, err);
        break;
      case MPPI_FAMILY_PIPELINE:
        st = bz == 1 ? launchPipeline<1>(args, stream, err) : launchPipeline<2>(args, stream, err);
        break;
      case MPPI_FAMILY_FUSED_REP:
        if constexpr (HAS_REP)
          forShape(FAST_SHAPES{}, bx, by, bz, [&](auto shape) {
            REP_T rep(dyn);
            st = launchFused(shape, rep, args, stream, err);
          });
        break;
      case MPPI_FAMILY_FUSED:
        forShape(SHAPES{}, bx, by, bz, [&](auto shape) { st = launchFused(shape, dyn, args, stream, err); });
        break;
      default:
        err = "block shape (" + std::to_string(bx) + "," + std::to_string(by) + "," + std::to_string(bz) +
              ") is not instantiated for this model";
        return MPPI_ERR_LAUNCH_SHAPE;
    }
    return noted(st, family, bx, by, bz, args.prev_records_d != nullptr);
  }

  /* ---- the single-rollout kernels (the trajectory re-roll of launchFinalize, launchReplay): a chain of T dependent steps, what
   *  counts is the length of a step's dependent chain ---- */
  enum SingleForm
  {
    FORM_WAVE,  ///< ONE rollout on a wave (HAS_WAVE); MPPI_AMD_FINALIZE_FORM=rep skips it — tests compare the two
    FORM_REP,   ///< the replicated-lane form: the register-resident single-wave variant
    FORM_OWN    ///< the model itself on FIN_BY contract lanes
  };
  /** The one choice of the form such a kernel runs on: the wave form, else the replicated-lane form if it is usable, each when
   *  its block fits the LDS, else the model itself.  bytes(form, which) is the block's LDS request on a form, launch(form, which,
   *  smem) launches on the chosen one; `which` is a std::integral_constant of SingleForm. */
  template <class BYTES, class LAUNCH>
  mppi_status onSingleRolloutForm(BYTES&& bytes, LAUNCH&& launch)
  {
    if constexpr (HAS_WAVE)
    {
      const char* env = getenv("MPPI_AMD_FINALIZE_FORM");
      if (!(env && env[0] == 'r'))
      {
        constexpr std::integral_constant<SingleForm, FORM_WAVE> which{};
        typename REP_T::FINALIZE_FORM wave(dyn);
        const size_t smem = bytes(wave, which);
        if (smem <= MAX_LDS_BYTES)
          return launch(wave, which, smem);
      }
    }
    if constexpr (HAS_REP)
    {
      if (repUsable())
      {
        constexpr std::integral_constant<SingleForm, FORM_REP> which{};
        REP_T rep(dyn);
        const size_t smem = bytes(rep, which);
        if (smem <= MAX_LDS_BYTES)
          return launch(rep, which, smem);
      }
    }
    constexpr std::integral_constant<SingleForm, FORM_OWN> which{};
    return launch(dyn, which, bytes(dyn, which));
  }
  mppi_status launchFinalize(int D, const kernels::FinalizeArgs& a, hipStream_t stream, std::string& err) override
  {
    if (!blobsReady(err))
      return MPPI_ERR_STATE;
    const bool scratch = a.scratch_d != nullptr;
    return onSingleRolloutForm(
        [&](auto& form, auto which) {
          if constexpr (decltype(which)::value == FORM_OWN)
            return kernels::finalizeSharedBytes(form, a.num_timesteps, FIN_BY, scratch);
          else
            return kernels::finalizeRepSharedBytes(form, a.num_timesteps, scratch);
        },
        [&](auto& form, auto which, size_t smem) -> mppi_status {
          using FORM_T = std::decay_t<decltype(form)>;
          if constexpr (decltype(which)::value == FORM_OWN)
          {
            if (smem > MAX_LDS_BYTES)
              return refuse(MPPI_ERR_LDS_OVERFLOW, "finalize kernel LDS overflow", err);
            auto kfn = scratch ? kernels::finalizeKernel<FORM_T, FIN_BY, true> : kernels::finalizeKernel<FORM_T, FIN_BY, false>;
            return launchChecked("finalizeKernel", kfn, dim3(D), dim3(kernels::finalizeBlockX(FIN_BY), FIN_BY, 1), smem, stream, err,
                                 form, a);
          }
          else
          {
            auto kfn = scratch ? kernels::finalizeRepKernel<FORM_T, true> : kernels::finalizeRepKernel<FORM_T, false>;
            return launchChecked(decltype(which)::value == FORM_WAVE ? "finalizeRepKernel (wave form)" : "finalizeRepKernel", kfn,
                                 dim3(D), dim3(64, 1, 1), smem, stream, err, form, a);
          }
        });
  }

  /** plain one-wave finalize form only (FIN_BY == 1, no replicated-lane / wave form): what the one-lane pipeline models have */
  static constexpr bool MERGE_CONTROL = FIN_BY == 1 && std::is_void<DYN_FAST_T>::value;
  bool supportsMergeControl(int num_timesteps) const override
  {
    if constexpr (MERGE_CONTROL)
      return kernels::mergeControlSharedBytes(dyn, num_timesteps) <= MAX_LDS_BYTES;
    return false;
  }
  mppi_status launchMergeControl(const kernels::FinalizeArgs& a, const kernels::MergeControlArgs& m, hipStream_t stream,
                                 std::string& err) override
  {
    if constexpr (MERGE_CONTROL)
    {
      if (!blobsReady(err))
        return MPPI_ERR_STATE;
      if (a.scratch_d || a.phases != 1 || ((a.num_timesteps * DYN_T::CONTROL_DIM) & 3) != 0 || m.num_records > 256)
        return refuse(MPPI_ERR_LAUNCH_SHAPE,
                      "mergeControlKernel: control phase of a split hand-over, sequence in LDS, T*C a multiple of 4, <= 256 records", err);
      const size_t smem = kernels::mergeControlSharedBytes(dyn, a.num_timesteps);
      return launchChecked("mergeControlKernel", kernels::mergeControlKernel<DYN_T>, dim3(1),
                           dim3(64 * kernels::MERGE_CONTROL_WAVES, 1, 1), smem, stream, err, dyn, a, m);
    }
    return refuse(MPPI_ERR_LAUNCH_SHAPE, "model has no merging control phase", err);
  }

  mppi_status launchModelStep(float* x_d, float* u_d, float dt, int enforce, hipStream_t stream,
                              std::string& err) override
  {
    if (!blobsReady(err))
      return MPPI_ERR_STATE;
    constexpr int Sd = DYN_T::STATE_DIM, Cd = DYN_T::CONTROL_DIM, Od = DYN_T::OUTPUT_DIM;
    const size_t smem = calcClassSharedMemSize(&dyn, 1) +
                        sizeof(float) * (3 * math::nearest_multiple_4(Sd) + math::nearest_multiple_4(Cd) +
                                         math::nearest_multiple_4(Od));
    return launchChecked("modelStepKernel", modelStepKernel<DYN_T, FIN_BY>, dim3(1), dim3(1, FIN_BY, 1), smem, stream, err, dyn, x_d,
                         u_d, dt, enforce);
  }

  bool hasComputeGrad() const override
  {
    return mppi::has_compute_grad<DYN_T>::value;
  }
  mppi_status launchLinearize(const kernels::LinearizeArgs& a, hipStream_t stream, std::string& err) override
  {
    if constexpr (mppi::has_compute_grad<DYN_T>::value)
    {
      // of the model's bulk data only the network weights enter the Jacobians (a costmap may still be missing): whichever form of
      // a model is the DYN_T here says where they are with gradWeights()
      if constexpr (has_grad_weights<DYN_T>::value)
        if (!dyn.gradWeights())
          return refuse(MPPI_ERR_STATE, "model needs the 'dynamics_weights' blob (mppi_set_model_blob) before it can be linearised", err);
      if (a.n < 1 || !a.x_d || !a.u_d || !a.A_d || !a.B_d)
        return refuse(MPPI_ERR_INVALID_ARG, "linearizeKernel: n >= 1 points and four device pointers", err);
      const size_t smem = kernels::linearizeSharedBytes(dyn);
      constexpr int P = kernels::linearizeBlockPoints<DYN_T>();
      return launchChecked("linearizeKernel", kernels::linearizeKernel<DYN_T>, dim3((a.n + P - 1) / P),
                           dim3(64 * kernels::linearizeBlockWaves<DYN_T>(), 1, 1), smem, stream, err, dyn, a,
                           kernels::linearizeModelSharedBytes(dyn));
    }
    return ModelBase::launchLinearize(a, stream, err);
  }
  mppi_status launchDdpBackward(const kernels::DdpBackwardArgs& a, hipStream_t stream, std::string& err) override
  {
    if constexpr (mppi::has_compute_grad<DYN_T>::value)
    {
      if (a.T < 1 || !a.A_d || !a.B_d || !a.Q_d || !a.R_d || !a.Qf_d || !a.gains_d || !a.status_d)
        return refuse(MPPI_ERR_INVALID_ARG, "ddpBackwardKernel: T >= 1 steps and seven device pointers", err);
      return launchChecked("ddpBackwardKernel", kernels::ddpBackwardKernel<DYN_T::STATE_DIM, DYN_T::CONTROL_DIM>, dim3(1),
                           dim3(64, 1, 1), 0, stream, err, a);
    }
    return ModelBase::launchDdpBackward(a, stream, err);
  }

  /** replayKernel on the form launchFinalize's re-roll runs on (onSingleRolloutForm chooses for both) */
  mppi_status launchReplay(const kernels::ReplayArgs& a, const SamplerLaunchState& s, hipStream_t stream, std::string& err) override
  {
    if (!blobsReady(err))
      return MPPI_ERR_STATE;
    if (a.n < 1 || !a.x0_d || !a.optimal_d || !a.idx_d || !a.y_d || !a.cost_d || !a.crash_d)
      return refuse(MPPI_ERR_INVALID_ARG, "replayKernel: n >= 1 rows and six device pointers", err);
    // the sampler as the last rollout launch saw it, on a copy: the model's own keeps what that launch left in it
    const SAMPLING_T keep = smp;
    prepSampler(s);
    const SAMPLING_T rs = smp;
    smp = keep;
    return onSingleRolloutForm(
        [&](auto& rd, auto which) { return kernels::replaySharedBytes(rd, cost, decltype(which)::value == FORM_OWN ? FIN_BY : 1); },
        [&](auto& rd, auto which, size_t smem) -> mppi_status {
          using RD_T = std::decay_t<decltype(rd)>;
          constexpr int BY = decltype(which)::value == FORM_OWN ? FIN_BY : 1;  // contract lanes per row
          const char* const what[] = {"replayKernel (wave form)", "replayKernel (replicated lanes)", "replayKernel"};
          if (smem > MAX_LDS_BYTES)
            return ldsOverflow(what[which], smem, err);
          constexpr int ROWS = BY == 1 ? kernels::replayBlockRows<RD_T>() : 1;
          return launchChecked(what[which], kernels::replayKernel<RD_T, COST_T, SAMPLING_T, BY>, dim3((a.n + ROWS - 1) / ROWS),
                               dim3(BY == 1 ? 64 : 1, BY, 1), smem, stream, err, rd, cost, rs, a);
        });
  }

  /** evaluateKernel on the same form; no sampler is involved */
  mppi_status launchEvaluate(const kernels::EvaluateArgs& a, hipStream_t stream, std::string& err) override
  {
    if (!blobsReady(err))
      return MPPI_ERR_STATE;
    if (a.n < 1 || a.num_timesteps < 1 || !a.x0_d || !a.u_d || !a.cost_d || !a.crash_d ||
        (a.x0_stride != 0 && a.x0_stride != DYN_T::STATE_DIM))
      return refuse(MPPI_ERR_INVALID_ARG, "evaluateKernel: n >= 1 rows, T >= 1 steps, four device pointers, a state stride of 0 or S",
                    err);
    return onSingleRolloutForm(
        [&](auto& rd, auto which) { return kernels::evaluateSharedBytes(rd, cost, decltype(which)::value == FORM_OWN ? FIN_BY : 1); },
        [&](auto& rd, auto which, size_t smem) -> mppi_status {
          using RD_T = std::decay_t<decltype(rd)>;
          constexpr int BY = decltype(which)::value == FORM_OWN ? FIN_BY : 1;  // contract lanes per row
          const char* const what[] = {"evaluateKernel (wave form)", "evaluateKernel (replicated lanes)", "evaluateKernel"};
          if (smem > MAX_LDS_BYTES)
            return ldsOverflow(what[which], smem, err);
          constexpr int ROWS = BY == 1 ? kernels::evaluateBlockRows<RD_T>() : 1;
          return launchChecked(what[which], kernels::evaluateKernel<RD_T, COST_T, BY>, dim3((a.n + ROWS - 1) / ROWS),
                               dim3(BY == 1 ? 64 : 1, BY, 1), smem, stream, err, rd, cost, a);
        });
  }
};

}  // namespace engine
}  // namespace mppi

#endif
