/**
 * ddp_feedback.hpp — device side of the DDP tracking controller used by Robust MPPI: u_fb = K_t (x - x*).
 *
 * reference: include/mppi/feedback_controllers/DDP/ddp.cuh:18-60 (DDPFeedbackState: fb_gain_traj_[T][S][C], i.e. the
 * C x S Eigen gain matrix of every timestep, column-major) and ddp.cu:11-45 (DeviceDDPImpl::k).
 * The gains arrive through the C ABI — from the caller (mppi_set_feedback_gains) or from the engine's own backward pass
 * (mppi_compute_feedback; ddp_backward.hpp, engine/feedback_kernel.hpp) — and live in one device buffer owned by the engine.
 *
 * Reference quirk, kept by default: for an even CONTROL_DIM ddp.cu:27-37 ASSIGNS `control_output = gain_row * e` inside
 * the loop over the states instead of accumulating, so only the LAST state's gain row survives
 * (u_fb[j] = K[S-1][j] * (x[S-1] - x*[S-1])); for an odd CONTROL_DIM it accumulates over all states (:39-43).
 * accumulate_all_states_ = true gives the mathematically intended sum over all states for every CONTROL_DIM.
 */
#ifndef MPPI_AMD_DDP_FEEDBACK_HPP_
#define MPPI_AMD_DDP_FEEDBACK_HPP_

#include <hip/hip_runtime.h>
#include "mppi_amd/plugin/managed.hpp"

namespace mppi
{
template <class DYN_T>
class DeviceDDP : public Managed
{
public:
  static const int STATE_DIM = DYN_T::STATE_DIM;
  static const int CONTROL_DIM = DYN_T::CONTROL_DIM;

  const float* fb_gain_traj_d_ = nullptr;  ///< [T][S][C] (device pointer owned by the engine)
  int num_timesteps_ = 0;
  bool accumulate_all_states_ = false;     ///< false: the reference's behaviour (see the header comment)

  __host__ __device__ int getGrdSharedSizeBytes() const
  {
    return 0;
  }
  __host__ __device__ int getBlkSharedSizeBytes() const
  {
    return 0;
  }
  /** reference: feedback_controllers/feedback.cuh initializeFeedback — nothing to set up for DDP gains */
  __device__ inline void initializeFeedback(const float* x, const float* u, float* theta_fb, const float t, const float dt)
  {
  }

  /** true when k() depends on the LAST state only (the reference's behaviour for an even CONTROL_DIM, see above): kernels
   *  that hand the nominal state from wave to wave then move one float per step instead of STATE_DIM */
  __device__ inline bool lastStateOnly() const
  {
    return (CONTROL_DIM % 2 == 0) && !accumulate_all_states_;
  }
  /** k() for lastStateOnly(): the assignment of the last state's term is the one that survives ddp.cu:27-37 */
  __device__ inline void kLastState(const float x_act_last, const float x_goal_last, const int t,
                                    float* __restrict__ control_output) const
  {
    const float* fb_gain_t = fb_gain_traj_d_ + (size_t)STATE_DIM * CONTROL_DIM * t + (STATE_DIM - 1) * CONTROL_DIM;
    const float e = x_act_last - x_goal_last;
#pragma unroll
    for (int j = 0; j < CONTROL_DIM; j++)
      control_output[j] = fb_gain_t[j] * e;
  }

  /** reference: ddp.cu:11-45.  control_output must be zero-initialised by the caller (rmppi_kernels.cu:755-758). */
  __device__ inline void k(const float* __restrict__ x_act, const float* __restrict__ x_goal, const int t,
                           float* __restrict__ theta, float* __restrict__ control_output) const
  {
    const float* fb_gain_t = fb_gain_traj_d_ + (size_t)STATE_DIM * CONTROL_DIM * t;
    const bool assign = (CONTROL_DIM % 2 == 0) && !accumulate_all_states_;
#pragma unroll
    for (int i = 0; i < STATE_DIM; i++)
    {
      const float e = x_act[i] - x_goal[i];
#pragma unroll
      for (int j = 0; j < CONTROL_DIM; j++)
      {
        const float term = fb_gain_t[i * CONTROL_DIM + j] * e;
        control_output[j] = assign ? term : control_output[j] + term;
      }
    }
  }
};
}  // namespace mppi

#include <functional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "mppi_amd.h"
#include "mppi_amd/plugin/host_arrays.hpp"

/**
 * DDPParams of the reference (feedback_controllers/DDP/ddp.cuh: Q, R, Q_f, num_iterations), on the plain host containers of
 * plugin/host_arrays.hpp instead of Eigen: Q(i, j), R(i, j), Q_f(i, j) as there.  Defaults as there: identities, one iteration.
 */
template <class DYN_T>
struct DDPParams
{
  mppi::host::Matrix<DYN_T::STATE_DIM, DYN_T::STATE_DIM> Q, Q_f;
  mppi::host::Matrix<DYN_T::CONTROL_DIM, DYN_T::CONTROL_DIM> R;
  int num_iterations = 1;
  DDPParams()
  {
    Q.setZero();
    Q_f.setZero();
    R.setZero();
    for (int i = 0; i < DYN_T::STATE_DIM; i++)
      Q(i, i) = Q_f(i, i) = 1.0f;
    for (int i = 0; i < DYN_T::CONTROL_DIM; i++)
      R(i, i) = 1.0f;
  }
};

/**
 * Host side of the DDP tracking controller with the reference's name, constructor and methods (feedback_controllers/DDP/ddp.cuh:
 * 62-140: DDPFeedback<DYN_T, NUM_TIMESTEPS>(model, dt), setParams, computeFeedback), so that a caller's
 * `new DDPFeedback<Dyn, T>(model, dt)` and the FB_T template argument of the controller classes keep compiling.  The gains are
 * handed in — setFeedbackGains(K[T][S][C]) — or computed: computeFeedback(init_state, goal_traj, control_traj) runs the backward
 * pass of the reference's solver (ddp/ddp.h with num_iterations = 1) on the device through the controller's engine handle
 * (mppi_compute_feedback_at; the controller binds its handle when it creates it) and stores the result where setFeedbackGains
 * does.  Either way a Robust controller uploads them before its next computeControl.
 * The linearisation points are (goal_traj, control_traj) themselves; the reference re-rolls the states from init_state with an
 * explicit Euler step and clamped controls (ddp.h:61-71) and linearises there — DESIGN.md §7.  init_state is accepted for the
 * reference's signature.
 */
template <class DYN_T, int NUM_TIMESTEPS>
class DDPFeedback
{
public:
  static const int FB_TIMESTEPS = NUM_TIMESTEPS;
  typedef DYN_T DYN_TYPE;
  typedef mppi::host::Array<DYN_T::STATE_DIM> state_array;
  typedef mppi::host::Matrix<DYN_T::STATE_DIM, NUM_TIMESTEPS> state_trajectory;
  typedef mppi::host::Matrix<DYN_T::CONTROL_DIM, NUM_TIMESTEPS> control_trajectory;
  DDPFeedback(DYN_T* model, float dt) : model_(model), dt_(dt)
  {
  }
  /** gains [T][S][C]: the C x S gain matrix of every time step, column-major (DDPFeedbackState::fb_gain_traj_) */
  void setFeedbackGains(const std::vector<float>& gains, bool accumulate_all_states = false)
  {
    gains_ = gains;
    accumulate_all_states_ = accumulate_all_states;
    version_++;
  }
  const std::vector<float>& getFeedbackGains() const
  {
    return gains_;
  }
  bool accumulateAllStates() const
  {
    return accumulate_all_states_;
  }
  unsigned version() const
  {
    return version_;
  }
  float getDt() const
  {
    return dt_;
  }
  /** reference: ddp.cu:81-88; takes effect at the next computeFeedback.  num_iterations other than 1 makes that call throw. */
  void setParams(const DDPParams<DYN_T>& params)
  {
    params_ = params;
    params_pushed_ = false;
  }
  DDPParams<DYN_T> getParams() const
  {
    return params_;
  }
  /** the engine handle computeFeedback works through, its horizon, and what brings the handle up to date with the caller's
   *  plugin objects (model parameters, control ranges) before a computation: the controller this object was given to calls it
   *  (nullptr: unbound) */
  void bindHandle(mppi_handle h, int num_timesteps, std::function<void()> sync = std::function<void()>())
  {
    h_ = h;
    num_timesteps_ = num_timesteps;
    sync_ = std::move(sync);
    params_pushed_ = false;
  }
  /** reference: ddp.cu:90-120.  goal_traj, control_traj: column t = time step t, the controller's num_timesteps of them. */
  template <class STATE_T, class STATE_TRAJ_T, class CONTROL_TRAJ_T>
  void computeFeedback(const STATE_T& init_state, const STATE_TRAJ_T& goal_traj, const CONTROL_TRAJ_T& control_traj)
  {
    static_assert(STATE_TRAJ_T::rows() == DYN_T::STATE_DIM && CONTROL_TRAJ_T::rows() == DYN_T::CONTROL_DIM,
                  "DDPFeedback::computeFeedback: trajectories of the model's state and control dimensions");
    if (num_timesteps_ > STATE_TRAJ_T::cols() || num_timesteps_ > CONTROL_TRAJ_T::cols())
      throw std::runtime_error("DDPFeedback::computeFeedback: the trajectories are shorter than the controller's horizon");
    (void)init_state;
    if (!h_)
      throw std::runtime_error("DDPFeedback::computeFeedback: no controller has bound its engine handle to this object yet");
    constexpr int S = DYN_T::STATE_DIM, C = DYN_T::CONTROL_DIM;
    if (sync_)
      sync_();
    if (!params_pushed_)
    {
      float Q[S * S], R[C * C], Qf[S * S];  // row-major for the C ABI
      for (int i = 0; i < S; i++)
        for (int j = 0; j < S; j++)
        {
          Q[i * S + j] = params_.Q(i, j);
          Qf[i * S + j] = params_.Q_f(i, j);
        }
      for (int i = 0; i < C; i++)
        for (int j = 0; j < C; j++)
          R[i * C + j] = params_.R(i, j);
      check(mppi_set_feedback_params(h_, Q, R, Qf, params_.num_iterations));
      params_pushed_ = true;
    }
    std::vector<float> g((size_t)num_timesteps_ * S * C);
    check(mppi_compute_feedback_at(h_, goal_traj.data(), control_traj.data(), g.data()));
    gains_.swap(g);
    version_++;
  }
  DYN_T* model_ = nullptr;

private:
  void check(mppi_status s) const
  {
    if (s != MPPI_OK)
      throw std::runtime_error(std::string(mppi_status_string(s)) + ": " + mppi_last_error(h_));
  }
  float dt_ = 0.0f;
  std::vector<float> gains_;
  bool accumulate_all_states_ = false;
  unsigned version_ = 0;
  DDPParams<DYN_T> params_;
  bool params_pushed_ = false;
  mppi_handle h_ = nullptr;
  int num_timesteps_ = 0;
  std::function<void()> sync_;
};
#endif
