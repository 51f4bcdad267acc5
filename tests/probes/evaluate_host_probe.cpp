// Stand-alone driver of include/mppi_amd/engine/evaluate_host.hpp (argument checks of mppi_evaluate_controls / mppi_warm_start and
// the warm-start choice rule), built by tests/test_evaluate_host.py plain and with -fsanitize=address,undefined.  One case per
// input line, one answer per output line:
//   args <x0 0|1> <x0_count> <u 0|1> <n>             -> "ok" or the refusal of checkEvaluateArgs
//   warm <x0 0|1> <candidates 0|1> <n> <hyst bits>   -> "ok" or the refusal of checkWarmStartArgs
//   choice <hyst bits> <n> <bits of costs[0..n]>     -> warmStartChoice
//   robust                                           -> the text a Robust handle is refused with
// Floats travel as the hexadecimal bit patterns of their float32 value.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "mppi_amd/engine/evaluate_host.hpp"

static float fromBits(const std::string& hex)
{
  const uint32_t b = (uint32_t)std::stoul(hex, nullptr, 16);
  float f;
  std::memcpy(&f, &b, sizeof(f));
  return f;
}

int main()
{
  using namespace mppi::evaluate;
  static const float there[4] = { 0.0f, 0.0f, 0.0f, 0.0f };  // what a non-null pointer points at; never read by the checks
  std::string line;
  while (std::getline(std::cin, line))
  {
    std::istringstream in(line);
    std::string kind;
    in >> kind;
    if (kind == "args")
    {
      int x0 = 0, x0_count = 0, u = 0, n = 0;
      in >> x0 >> x0_count >> u >> n;
      const std::string r = checkEvaluateArgs(x0 ? there : nullptr, x0_count, u ? there : nullptr, n);
      std::printf("%s\n", r.empty() ? "ok" : r.c_str());
    }
    else if (kind == "warm")
    {
      int x0 = 0, cand = 0, n = 0;
      std::string hyst;
      in >> x0 >> cand >> n >> hyst;
      const std::string r = checkWarmStartArgs(x0 ? there : nullptr, cand ? there : nullptr, n, fromBits(hyst));
      std::printf("%s\n", r.empty() ? "ok" : r.c_str());
    }
    else if (kind == "choice")
    {
      std::string hyst, bits;
      int n = 0;
      in >> hyst >> n;
      std::vector<float> costs;
      while (in >> bits)
        costs.push_back(fromBits(bits));
      if (n < 1 || (int)costs.size() != n + 1)
      {
        std::printf("bad case\n");
        return 2;
      }
      std::printf("%d\n", warmStartChoice(costs.data(), n, fromBits(hyst)));
    }
    else if (kind == "robust")
      std::printf("%s\n", warmStartRobustRefusal());
    else if (!kind.empty())
    {
      std::printf("bad case\n");
      return 2;
    }
  }
  return 0;
}
