/**
 * ddp_backward_sanitized.cpp — TEST CODE: the host recursion of include/mppi_amd/feedback_controllers/ddp_backward.hpp at S = 13,
 * C = 4, T = 3 in a stand-alone program, for a build with the address and undefined-behaviour sanitizers (nothing sanitized is
 * loaded into Python; not part of the pytest suite):
 *   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tests/probes/ddp_backward_sanitized.cpp
 *       -o examples/_build/ddp_backward_sanitized && examples/_build/ddp_backward_sanitized
 * Every array is an exact-size heap allocation, so a read or write one entry past any of them is reported.  Prints "ok <failing step> <float64 sum of the gains>"; exit status 0 when the pass succeeded, wrote
 * row T - 1 as zeros and left the guard pattern of no row standing.
 */
#include <cmath>
#include <cstdio>
#include <vector>

#include "mppi_amd/feedback_controllers/ddp_backward.hpp"

int main()
{
  constexpr int S = 13, C = 4, T = 3;
  std::vector<float> A((size_t)T * S * S), B((size_t)T * S * C), Q((size_t)S * S, 0.0f), R((size_t)C * C, 0.0f), Qf((size_t)S * S, 0.0f);
  unsigned s = 12345u;
  auto next = [&s]() {
    s = s * 1664525u + 1013904223u;
    return (float)((s >> 8) & 0xFFFF) / 65536.0f - 0.5f;
  };
  for (float& v : A)
    v = 2.0f * next();
  for (float& v : B)
    v = 2.0f * next();
  for (int i = 0; i < S; i++)
  {
    Q[i * S + i] = 1.0f + (float)i;
    Qf[i * S + i] = 2.0f;
  }
  Qf[1] = 0.5f;  // not symmetric: symmetrised on entry
  for (int i = 0; i < C; i++)
    R[i * C + i] = 1.0f;
  std::vector<float> gains((size_t)T * S * C, -77.0f);
  int fail_step = -5;
  const bool ok = mppi::ddp::backwardPass<S, C>(A.data(), B.data(), Q.data(), R.data(), Qf.data(), 0.02f, T, gains.data(), &fail_step);
  double sum = 0.0;
  bool clean = ok && fail_step == -1;
  for (size_t i = 0; i < gains.size(); i++)
  {
    sum += (double)gains[i];
    clean = clean && std::isfinite(gains[i]) && gains[i] != -77.0f;
    if (i >= (size_t)(T - 1) * S * C)
      clean = clean && gains[i] == 0.0f;
  }
  printf("%s %d %.17g\n", ok ? "ok" : "failed", fail_step, sum);
  return clean ? 0 : 1;
}
