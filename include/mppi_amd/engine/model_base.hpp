/**
 * model_base.hpp — the interface libmppi_amd.so and a model translation unit share: ModelBase, the structures that cross it, and
 * the fingerprint mppi_register_model compares.  ModelT (model_instance.hpp) is its one implementation.
 */
#ifndef MPPI_AMD_MODEL_BASE_HPP_
#define MPPI_AMD_MODEL_BASE_HPP_

#include <hip/hip_runtime.h>
#include <cmath>
#include <string>
#include <vector>

#include "mppi_amd.h"
#include "rollout_kernel.hpp"
#include "finalize_kernel.hpp"
#include "rmppi_kernels.hpp"
#include "linearize_kernel.hpp"
#include "feedback_kernel.hpp"
#include "replay_kernel.hpp"
#include "evaluate_kernel.hpp"

namespace mppi
{
namespace engine
{
/** everything the sampler needs to know for one launch (the engine refreshes it before every launch) */
struct SamplerLaunchState
{
  int num_rollouts_local, num_rollouts_global, rollout_offset;
  int num_timesteps, num_distributions;
  float* control_means_d;
  const float* eps_d;  // nullptr => Philox
  float* control_samples_d;
  uint64_t seed;
  uint32_t generation;
  int iteration;  // opt_iter for std_dev_decay
  int optimization_stride;
  int independent_noise;  // != 0: use_same_noise_for_all_distributions off (every distribution its own stream / eps slab)
};

/** what the most recent rollout launch of a model object ran (mppi_get_launch_info): written by the dispatch itself, at the
 *  point where it has picked the kernel and the launch went out, so the query never recomputes the choice */
struct LaunchRecord
{
  int family = MPPI_FAMILY_NONE;  ///< mppi_kernel_family
  int bx = 0, by = 0, bz = 0;     ///< the registered block shape the launch was dispatched for
  bool rows_in_hbm = false;       ///< the sampler's rows in HBM (setGlobalRows)
  bool streamed_merge = false;    ///< the sampler waves merged the previous launch's block records (STREAM_MERGE form)
};

struct ModelBase
{
  int S = 0, C = 0, O = 0;
  int default_bx = 64, default_by = 1;
  LaunchRecord last_launch;
  virtual ~ModelBase() = default;
  virtual mppi_status setDynamicsParams(const void* pod, size_t n) = 0;
  virtual mppi_status setCostParams(const void* pod, size_t n) = 0;
  virtual void setControlRanges(const float* lo_hi) = 0;
  virtual void setControlDeadband(const float* db) = 0;
  virtual void getZeroControl(float* out) const = 0;
  /** Dynamics::enforceLeash (dynamics/dynamics.cuh:448-466), host: per state dimension, the nominal state if it is within
   *  the leash of the true state, else the true state moved towards it by the leash.  A plugin with an enforceLeash() host
   *  method of its own (RacerDubins: position leash in the body frame, racer_dubins.cu:177-230) overrides it. */
  virtual void hostEnforceLeash(const float* state_true, const float* state_nominal, const float* leash, float* out) const
  {
    for (int i = 0; i < S; i++)
    {
      const float diff = fabsf(state_nominal[i] - state_true[i]);
      if (leash[i] < diff)
        out[i] = state_true[i] + fminf(fmaxf(state_nominal[i] - state_true[i], -leash[i]), leash[i]);
      else
        out[i] = state_nominal[i];
    }
  }
  /** the base enforceConstraints rule on the host (dynamics.cu:97-116); false: the plugin overrides it, run the device code */
  virtual bool hostEnforceConstraints(float* u) const = 0;
  virtual void setSamplerParams(const mppi_gaussian_params* p, int D) = 0;
  /** bulk data (NN weights, costmap); default: the model has none */
  virtual mppi_status setBlob(const std::string& name, const float* data, size_t count, const int* dims, int ndims,
                              hipStream_t stream, std::string& err)
  {
    err = "model has no blob named '" + name + "'";
    return MPPI_ERR_INVALID_ARG;
  }
  /** LSTMHelper::copyHiddenCellToDevice (lstm_helper.cu:480-500): new initial hidden / cell state of the rollouts' LSTM,
   *  on the engine's stream without re-uploading the weights; default: the model has no LSTM */
  virtual mppi_status setLSTMInitialState(const float* hidden, const float* cell, hipStream_t stream, std::string& err)
  {
    err = "model has no LSTM";
    return MPPI_ERR_INVALID_ARG;
  }
  /** time_specific_std_dev: sigma[D][T][C] table in device memory (owned by the engine), nullptr switches it off */
  virtual void setTimeSpecificStdDev(const float* table_d) = 0;
  /** colored-noise sampler parameters (ColoredNoiseParamsImpl, colored_noise.cuh:45-73); default: Gaussian sampler */
  virtual mppi_status setColoredNoiseParams(const float* exponents, float offset_decay_rate, float fmin)
  {
    return MPPI_ERR_STATE;
  }
  /** floats of injected noise per rollout: T*C time-domain eps, or C*(2T+2) spectrum entries for colored noise */
  virtual size_t noiseFloatsPerRollout(int T) const = 0;
  /** the sampled noise eps[K_local][T][C] the next launch would use, written to out_d (generator parity tests) */
  virtual mppi_status launchNoiseDump(const SamplerLaunchState& s, float* out_d, hipStream_t stream, std::string& err) = 0;
  /* ---- Robust MPPI (rmppi_kernels.hpp); default: the model is not instantiated for it ---- */
  virtual bool supportsRMPPI() const
  {
    return false;
  }
  /** DDP feedback gains [T][S][C] (ddp.cuh:18-60) -> the model's device buffer; accumulate_all_states: see ddp_feedback.hpp;
   *  gains_on_device: `gains` is device memory (the output of launchDdpBackward), copied on `stream` device to device */
  virtual mppi_status setFeedbackGains(const float* gains, int T, bool accumulate_all_states, bool gains_on_device,
                                       hipStream_t stream, std::string& err)
  {
    err = "model is not instantiated for Robust MPPI";
    return MPPI_ERR_UNSUPPORTED;
  }
  virtual mppi_status launchInitEval(bool pipeline, const kernels::InitEvalArgs& a, const SamplerLaunchState& s,
                                     hipStream_t stream, std::string& err)
  {
    err = "model is not instantiated for Robust MPPI";
    return MPPI_ERR_UNSUPPORTED;
  }
  /** pipeline: the role-pipelined kernel (rmppi_pipeline_kernel.hpp) when the model has one and its replicated-lane form is
   *  usable with the loaded networks, else rolloutRMPPIKernel */
  virtual mppi_status launchRMPPI(int bx, bool pipeline, const kernels::RMPPIArgs& a, const SamplerLaunchState& s,
                                  hipStream_t stream, std::string& err)
  {
    err = "model is not instantiated for Robust MPPI";
    return MPPI_ERR_UNSUPPORTED;
  }
  virtual size_t rmppiSharedBytes(int bx, int T)
  {
    return 0;
  }
  /** LDS request of the role-pipelined Robust MPPI kernel (64 rollouts x 2 systems per block); 0: the model has none, its
   *  replicated-lane form does not take the loaded networks, or not even the shortest rings fit */
  virtual size_t rmppiPipelineSharedBytes(int T)
  {
    return 0;
  }
  /** world -> texture transform of a costmap cost (ARStandardCost::updateTransform, ar_standard_cost.cu:132-137) */
  virtual mppi_status setCostmapTransform(const float* r_c1, const float* r_c2, const float* trs)
  {
    return MPPI_ERR_INVALID_ARG;
  }
  virtual bool supportsShape(int bx, int by, int bz) const = 0;
  /** role-pipelined variant (rollout_pipeline_kernel.hpp) available for this model? */
  virtual bool supportsPipeline() const
  {
    return false;
  }
  /** "" when every plugin class the model's ROLE-SEPARATED kernels would run declares MPPI_BARRIER_FREE_STEP
   *  (plugin/parallel_utils.hpp: barrier_free_step) — or when the model has no such kernels; otherwise the names the
   *  declaration is missing from.  mppi_create refuses a model with a non-empty answer: a block barrier inside a per-step
   *  method would hang those kernels (only the wave whose role it is calls the method). */
  virtual std::string undeclaredBarrierFreePlugins() const
  {
    return std::string();
  }
  /** rolloutPipelineKernel's STREAM_MERGE form exists: one system, Gaussian sampler drawing in the loop */
  virtual bool supportsStreamedMerge() const
  {
    return false;
  }
  /** role-pipelined variant with the two systems of Tube-MPPI folded into the lanes of a wave, shape (32, 1, 2) */
  virtual bool supportsPipelineFold(int bx, int by, int bz) const
  {
    return false;
  }
  /** role-pipelined variant for replicated-lane (MFMA) dynamics, shape (64, REP, 1) */
  virtual bool supportsPipelineRep(int bx, int by, int bz) const
  {
    return false;
  }
  /** the shape is a replicated-lane one that the model's present data rule out (networks of another shape than the
   *  replicated-lane form is compiled for) */
  virtual bool fastShapeRefused(int bx, int by, int bz) const
  {
    return false;
  }
  virtual size_t rolloutSharedBytes(int bx, int by, int bz, int T, int D, bool pipeline) = 0;
  /** floats the sampler needs for the sample rows of `blocks` blocks of `slots` rollout slots in HBM (long horizons), 0: the
   *  sampler keeps its rows in LDS only; setGlobalRows(ptr) switches the fused kernel over (nullptr: back to LDS) */
  virtual size_t globalRowsFloats(int blocks, int slots, int T) const
  {
    return 0;
  }
  virtual void setGlobalRows(float* rows_d)
  {
  }
  /** every registered block shape as (bx, by, bz) triples, flattened */
  virtual void listShapes(std::vector<int>& out) const = 0;
  virtual mppi_status launchRollout(int bx, int by, int bz, bool pipeline, const kernels::RolloutArgs& args,
                                    const SamplerLaunchState& s, hipStream_t stream, std::string& err) = 0;
  virtual mppi_status launchFinalize(int D, const kernels::FinalizeArgs& a, hipStream_t stream, std::string& err) = 0;
  /** the control phase of a split hand-over that merges the last launch's block records itself (kernels::mergeControlKernel):
   *  one system on the plain one-wave finalize form, control sequence in LDS */
  virtual bool supportsMergeControl(int num_timesteps) const
  {
    return false;
  }
  virtual mppi_status launchMergeControl(const kernels::FinalizeArgs& a, const kernels::MergeControlArgs& m, hipStream_t stream,
                                         std::string& err)
  {
    err = "model has no merging control phase";
    return MPPI_ERR_LAUNCH_SHAPE;
  }
  /** x <- one model step (optionally after enforceConstraints on u), one block (1, by, 1) */
  virtual mppi_status launchModelStep(float* x_d, float* u_d, float dt, int enforce, hipStream_t stream,
                                      std::string& err) = 0;
  /** the replicated-lane (MFMA / four-lane) block shapes among listShapes(), as (bx, by, bz) triples, flattened */
  virtual void listReplicatedLaneShapes(std::vector<int>& out) const
  {
  }
  /** the role-pipelined Robust MPPI kernel (rmppi_pipeline_kernel.hpp) is instantiated for this model */
  virtual bool supportsRMPPIPipeline() const
  {
    return false;
  }
  /** channels of the "costmap" blob of a cost with costmap_d_: 1 {height, width}, 4 {height, width, 4}; 0: the cost has none */
  virtual int costmapChannels() const
  {
    return 0;
  }
  /** the Dynamics class declares a device computeGrad (plugin/dynamics.hpp: has_compute_grad) */
  virtual bool hasComputeGrad() const
  {
    return false;
  }
  /** A[n][S][S], B[n][S][C] <- the model's Jacobians at the n points x[n][S], u[n][C], all in device memory: one launch of
   *  kernels::linearizeKernel on `stream` (engine/linearize_kernel.hpp); default: the model declares no computeGrad */
  virtual mppi_status launchLinearize(const kernels::LinearizeArgs& a, hipStream_t stream, std::string& err)
  {
    err = "the model's Dynamics class declares no computeGrad";
    return MPPI_ERR_UNSUPPORTED;
  }
  /** gains[T][S][C], status[2] <- the DDP backward pass over A[T][S][S], B[T][S][C] where launchLinearize left them: one launch of
   *  kernels::ddpBackwardKernel<S, C> on `stream` (engine/feedback_kernel.hpp); default as above */
  virtual mppi_status launchDdpBackward(const kernels::DdpBackwardArgs& a, hipStream_t stream, std::string& err)
  {
    err = "the model's Dynamics class declares no computeGrad";
    return MPPI_ERR_UNSUPPORTED;
  }
  /** a.n rows (saved samples, or the current control sequence) run again through the model's plugins, their outputs, step costs and
   *  crash flags kept: one launch of kernels::replayKernel on `stream` (engine/replay_kernel.hpp) in the lane form the model's
   *  trajectory re-roll uses; `s`: the sampler state of the last rollout launch with the means the likelihood-ratio term reads */
  virtual mppi_status launchReplay(const kernels::ReplayArgs& a, const SamplerLaunchState& s, hipStream_t stream, std::string& err)
  {
    err = "model has no replay kernel";
    return MPPI_ERR_UNSUPPORTED;
  }
  /** cost[a.n], crash[a.n] <- the trajectory cost (no likelihood-ratio term) and the last crash status of the a.n control sequences
   *  a.u_d the caller brought, each from its own or from one initial state: one launch of kernels::evaluateKernel on `stream`
   *  (engine/evaluate_kernel.hpp) in the lane form the model's trajectory re-roll uses */
  virtual mppi_status launchEvaluate(const kernels::EvaluateArgs& a, hipStream_t stream, std::string& err)
  {
    err = "model has no evaluate kernel";
    return MPPI_ERR_UNSUPPORTED;
  }
};

/** fingerprint of the structures a model translation unit and libmppi_amd.so exchange (mppi_register_model refuses a
 *  plugin built against other headers: its kernels would read the argument blocks with the wrong layout) */
/** bumped BY HAND whenever ModelBase's virtual methods are added, removed or reordered or a field of an argument struct is
 *  swapped at equal size — changes sizeof() cannot see (a stale plugin would dispatch to the wrong vtable slot).
 *  3: rows-in-HBM arguments; 4: release-flag arguments of the finalize kernels (both round 3); 5: supportsStreamedMerge (round 4);
 *  6: FinalizeArgs::phases / carry block of the split hand-over (round 5); 7: undeclaredBarrierFreePlugins; 8: the transposed
 *  record copy (RolloutArgs) and supportsMergeControl / launchMergeControl (both round 6); 9: LaunchRecord,
 *  listReplicatedLaneShapes / supportsRMPPIPipeline (the launch and model introspection of mppi_amd.h); 10: costmapChannels;
 *  11: hasComputeGrad / launchLinearize; 12: launchDdpBackward, setFeedbackGains' gains_on_device; 13: launchReplay;
 *  14: launchEvaluate. */
#define MPPI_ENGINE_ABI_VERSION 14

constexpr int engineAbiFingerprint()
{
  return MPPI_ENGINE_ABI_VERSION * 1000003 +
         (int)(sizeof(ModelBase) + 131 * sizeof(kernels::RolloutArgs) + 131 * 131 * sizeof(kernels::FinalizeArgs) +
               7 * sizeof(kernels::RMPPIArgs) + 17 * sizeof(kernels::InitEvalArgs) + 31 * sizeof(SamplerLaunchState) +
               37 * sizeof(kernels::MergeControlArgs) + 41 * sizeof(kernels::LinearizeArgs) +
               43 * sizeof(kernels::DdpBackwardArgs) + 47 * sizeof(kernels::ReplayArgs) +
               53 * sizeof(kernels::EvaluateArgs));
}

}  // namespace engine
}  // namespace mppi

#endif
