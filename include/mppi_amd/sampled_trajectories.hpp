/**
 * sampled_trajectories.hpp — the state behind the reference's sampled-trajectory API of Controller (controllers/controller.cuh:
 * 229-296, 724-778; controller.cu:55-179), shared by the host classes of controllers.hpp and controllers_templated.hpp:
 *   setTopNSampledControlTrajectories / setPercentageSampledControlTrajectories   what to replay
 *   calculateSampledStateTrajectories                                             mppi_top_rollouts + mppi_replay_rollouts
 *   getSampledOutputTrajectories / getSampledCostTrajectories / getSampledCrashStatusTrajectories / getTopNCosts
 * Row 0 is the optimal sequence, then the randomly drawn rollouts, then the top N (engine/replay_host.hpp: sampledTrajectoryList).
 * Rows other than row 0 need a handle created with cfg.save_samples.  getTopNCosts returns the raw trajectory costs in ascending
 * order (the reference divides by the normaliser and leaves the order to its host list).  Plain C++11, no HIP header.
 */
#ifndef MPPI_AMD_SAMPLED_TRAJECTORIES_HPP_
#define MPPI_AMD_SAMPLED_TRAJECTORIES_HPP_

#include <cstdint>
#include <vector>

#include "mppi_amd.h"
#include "mppi_amd/engine/replay_host.hpp"

namespace mppi_amd
{
struct SampledTrajectories
{
  int top_n = 0;
  float fraction = 0.0f;
  uint64_t seed = 42;
  std::vector<int> indices;    ///< the rows of the last calculation, local rollout indices (-1: the optimal sequence)
  std::vector<float> outputs;  ///< [rows][T][O] output after each step
  std::vector<float> costs;    ///< [rows][T + 1] step costs, the terminal cost last
  std::vector<int> crash;      ///< [rows][T]
  std::vector<int> top_indices;
  std::vector<float> top_costs;

  bool wantsSamples() const
  {
    return top_n > 0 || fraction > 0.0f;
  }
  /** selection, list, replay; the first failing status (the message is the handle's mppi_last_error) */
  mppi_status calculate(mppi_handle h, int num_timesteps, int output_dim, int system = 0)
  {
    int k_local = 0;
    mppi_status s = mppi_get_local_rollouts(h, &k_local, nullptr);
    if (s != MPPI_OK)
      return s;
    top_indices.assign((size_t)(top_n > 0 ? top_n : 0), 0);
    top_costs.assign(top_indices.size(), 0.0f);
    if (top_n > 0)
    {
      s = mppi_top_rollouts(h, system, top_n, top_indices.data(), top_costs.data());
      if (s != MPPI_OK)
        return s;
    }
    indices = mppi::replay::sampledTrajectoryList(k_local, (double)fraction, seed, top_indices.data(), (int)top_indices.size());
    const size_t n = indices.size();
    outputs.assign(n * (size_t)num_timesteps * (size_t)output_dim, 0.0f);
    costs.assign(n * (size_t)(num_timesteps + 1), 0.0f);
    crash.assign(n * (size_t)num_timesteps, 0);
    return mppi_replay_rollouts(h, system, indices.data(), (int)n, outputs.data(), costs.data(), crash.data());
  }
};
}  // namespace mppi_amd

#endif
