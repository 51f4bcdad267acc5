/**
 * evaluate_host.hpp — the host logic around mppi_evaluate_controls / mppi_warm_start that needs no device: the argument checks of
 * the two entry points and the rule by which a warm start keeps the current control sequence or installs a candidate.  Plain C++,
 * no HIP header: the engine and a stand-alone sanitizer build share it.
 */
#ifndef MPPI_AMD_ENGINE_EVALUATE_HOST_HPP_
#define MPPI_AMD_ENGINE_EVALUATE_HOST_HPP_

#include <cmath>
#include <string>

namespace mppi
{
namespace evaluate
{
constexpr int EVALUATE_N_MAX = 65536;                   ///< largest n of mppi_evaluate_controls
constexpr int WARM_START_N_MAX = EVALUATE_N_MAX - 1;  ///< largest n of mppi_warm_start: the current sequence is one more row

/** "" when 1 <= n <= EVALUATE_N_MAX, x0 and u are there and x0_count is 1 or n, else the refusal */
inline std::string checkEvaluateArgs(const float* x0, int x0_count, const float* u, int n)
{
  if (n < 1 || n > EVALUATE_N_MAX)
    return "mppi_evaluate_controls: n = " + std::to_string(n) + " is outside [1, " + std::to_string(EVALUATE_N_MAX) + "]";
  if (!x0)
    return "mppi_evaluate_controls: null x0";
  if (!u)
    return "mppi_evaluate_controls: null u";
  if (x0_count != 1 && x0_count != n)
    return "mppi_evaluate_controls: x0_count = " + std::to_string(x0_count) + " is neither 1 (one initial state for every row) nor n = " +
           std::to_string(n) + " (one per row)";
  return std::string();
}

/** "" when 1 <= n <= WARM_START_N_MAX, x0 and the candidates are there and the hysteresis is finite and >= 0, else the refusal */
inline std::string checkWarmStartArgs(const float* x0, const float* candidates, int n, float hysteresis)
{
  if (n < 1 || n > WARM_START_N_MAX)
    return "mppi_warm_start: n = " + std::to_string(n) + " is outside [1, " + std::to_string(WARM_START_N_MAX) + "]";
  if (!x0)
    return "mppi_warm_start: null x0";
  if (!candidates)
    return "mppi_warm_start: null candidates";
  if (!(hysteresis >= 0.0f) || std::isinf(hysteresis))
    return "mppi_warm_start: the hysteresis has to be finite and >= 0";
  return std::string();
}

/** what a Robust handle is told (MPPI_ERR_UNSUPPORTED) */
inline const char* warmStartRobustRefusal()
{
  return "mppi_warm_start: the nominal system of a Robust MPPI handle is chosen by its candidate-state search; installing a "
         "control sequence under it is not supported";
}

/** a orders before b in mppi_top_rollouts' order: ascending, NaN after every number (ties: the caller keeps the lower index) */
inline bool costBefore(float a, float b)
{
  if (std::isnan(a))
    return false;
  return std::isnan(b) || a < b;
}

/**
 * costs[n + 1]: the current control sequence's cost, then the n candidates'.  The cheapest candidate — ties to the lower index —
 * is returned if its cost is below current - hysteresis (strictly), or if the current cost is NaN and its own is not; else -1:
 * the current sequence stays.
 */
inline int warmStartChoice(const float* costs, int n, float hysteresis)
{
  int best = 0;
  for (int i = 1; i < n; i++)
    if (costBefore(costs[1 + i], costs[1 + best]))
      best = i;
  const float current = costs[0], c = costs[1 + best];
  if (std::isnan(c))
    return -1;
  if (std::isnan(current))
    return best;
  return c < current - hysteresis ? best : -1;
}

}  // namespace evaluate
}  // namespace mppi

#endif
