/**
 * replay_host.hpp — the host logic around mppi_top_rollouts / mppi_replay_rollouts that needs no device: the argument checks of
 * the two entry points and the list of rows the reference's Controller replays (controllers/controller.cu:55-179).  Plain C++,
 * no HIP header: the engine, the C++ host classes (controllers.hpp) and a stand-alone sanitizer build share it.
 */
#ifndef MPPI_AMD_ENGINE_REPLAY_HOST_HPP_
#define MPPI_AMD_ENGINE_REPLAY_HOST_HPP_

#include <cstdint>
#include <random>
#include <string>
#include <vector>

namespace mppi
{
namespace replay
{
constexpr int TOP_N_MAX = 256;     ///< largest n of mppi_top_rollouts (kernels::TOP_ROLLOUTS_MAX)
constexpr int REPLAY_N_MAX = 1024;  ///< largest n of mppi_replay_rollouts

/** "" when 1 <= n <= min(K_local, TOP_N_MAX), else the refusal */
inline std::string checkTopN(int n, int k_local)
{
  const int limit = k_local < TOP_N_MAX ? k_local : TOP_N_MAX;
  if (n < 1 || n > limit)
    return "mppi_top_rollouts: n = " + std::to_string(n) + " is outside [1, " + std::to_string(limit) +
           "] (the local rollouts, at most " + std::to_string(TOP_N_MAX) + ")";
  return std::string();
}

/** "" when 1 <= n <= REPLAY_N_MAX and every index is in [-1, K_local), else the refusal; needs_samples / needs_optimal: an
 *  index >= 0 / the index -1 occurs */
inline std::string checkReplayIndices(const int* idx, int n, int k_local, bool& needs_samples, bool& needs_optimal)
{
  needs_samples = needs_optimal = false;
  if (n < 1 || n > REPLAY_N_MAX)
    return "mppi_replay_rollouts: n = " + std::to_string(n) + " is outside [1, " + std::to_string(REPLAY_N_MAX) + "]";
  if (!idx)
    return "mppi_replay_rollouts: null index list";
  for (int i = 0; i < n; i++)
  {
    if (idx[i] < -1 || idx[i] >= k_local)
      return "mppi_replay_rollouts: rollout_idx[" + std::to_string(i) + "] = " + std::to_string(idx[i]) + " is outside [-1, " +
             std::to_string(k_local) + ") (local rollout indices; -1 is the current control sequence)";
    if (idx[i] < 0)
      needs_optimal = true;
    else
      needs_samples = true;
  }
  return std::string();
}

/** rows the random part of the list holds: int(fraction * K), as controller.cu:63 */
inline int sampledCount(double fraction, int k)
{
  if (!(fraction > 0.0) || k <= 0)
    return 0;
  const long long m = (long long)(fraction * (double)k);
  return (int)(m > k ? k : m);
}

/**
 * The list Controller::calculateSampledStateTrajectories replays (controller.cu:55-179): slot 0 the optimal sequence (-1), then
 * sampledCount(fraction, K) indices drawn without replacement from the first 98 % of the rollouts — the last ones are pure noise;
 * a fraction above 0.98 takes 0, 1, 2, ... instead (:65-69) — then the top-N indices the caller selected.  The draw is a partial
 * Fisher-Yates shuffle with a seeded std::mt19937_64; the list is cut at REPLAY_N_MAX rows.
 */
inline std::vector<int> sampledTrajectoryList(int k, double fraction, uint64_t seed, const int* top_idx, int n_top)
{
  std::vector<int> out;
  out.push_back(-1);
  const int m = sampledCount(fraction, k);
  if (m > 0)
  {
    if (fraction > 0.98)
    {
      for (int i = 0; i < m; i++)
        out.push_back(i);
    }
    else
    {
      const int pool_size = (int)((double)k * 0.98);
      std::vector<int> pool((size_t)(pool_size > 0 ? pool_size : 0));
      for (int i = 0; i < (int)pool.size(); i++)
        pool[(size_t)i] = i;
      std::mt19937_64 gen(seed);
      const int take = m < (int)pool.size() ? m : (int)pool.size();
      for (int i = 0; i < take; i++)
      {
        const size_t j = (size_t)i + (size_t)(gen() % (uint64_t)(pool.size() - (size_t)i));
        const int tmp = pool[(size_t)i];
        pool[(size_t)i] = pool[j];
        pool[j] = tmp;
        out.push_back(pool[(size_t)i]);
      }
    }
  }
  for (int i = 0; i < n_top && top_idx; i++)
    out.push_back(top_idx[i]);
  if (out.size() > (size_t)REPLAY_N_MAX)
    out.resize((size_t)REPLAY_N_MAX);
  return out;
}

}  // namespace replay
}  // namespace mppi

#endif
