// Stand-alone check of include/mppi_amd/engine/replay_host.hpp (argument checks of mppi_top_rollouts / mppi_replay_rollouts and
// the sampled-trajectory list), built by tests/test_replay_host.py with -fsanitize=address,undefined.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "mppi_amd/engine/replay_host.hpp"

#define EXPECT(cond)                                                   \
  do                                                                   \
  {                                                                    \
    if (!(cond))                                                       \
    {                                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      return 1;                                                        \
    }                                                                  \
  } while (0)

int main()
{
  using namespace mppi::replay;
  // n of a selection
  EXPECT(checkTopN(1, 65).empty() && checkTopN(65, 65).empty() && checkTopN(256, 1049).empty());
  EXPECT(!checkTopN(0, 65).empty() && !checkTopN(66, 65).empty() && !checkTopN(257, 1049).empty() && !checkTopN(-3, 65).empty());
  EXPECT(checkTopN(66, 65).find("[1, 65]") != std::string::npos);
  // index lists
  bool smp = false, opt = false;
  {
    std::vector<int> idx = { -1, 0, 64, 199 };
    EXPECT(checkReplayIndices(idx.data(), (int)idx.size(), 200, smp, opt).empty() && smp && opt);
    idx = { -1 };
    EXPECT(checkReplayIndices(idx.data(), 1, 200, smp, opt).empty() && !smp && opt);
    idx = { 5, 200 };
    const std::string e = checkReplayIndices(idx.data(), 2, 200, smp, opt);
    EXPECT(e.find("rollout_idx[1] = 200") != std::string::npos && e.find("[-1, 200)") != std::string::npos);
    idx = { -2 };
    EXPECT(!checkReplayIndices(idx.data(), 1, 200, smp, opt).empty());
    EXPECT(!checkReplayIndices(idx.data(), 0, 200, smp, opt).empty());
    EXPECT(!checkReplayIndices(nullptr, 3, 200, smp, opt).empty());
    std::vector<int> many((size_t)REPLAY_N_MAX + 1, 0);
    EXPECT(!checkReplayIndices(many.data(), (int)many.size(), 200, smp, opt).empty());
    EXPECT(checkReplayIndices(many.data(), REPLAY_N_MAX, 200, smp, opt).empty());
  }
  // the list: slot 0, the draw, the top N
  {
    const int top[3] = { 7, 3, 11 };
    std::vector<int> l = sampledTrajectoryList(1049, 0.0, 1, top, 3);
    EXPECT((l == std::vector<int>{ -1, 7, 3, 11 }));
    l = sampledTrajectoryList(1049, 0.05, 9, nullptr, 0);
    EXPECT((int)l.size() == 1 + sampledCount(0.05, 1049) && l[0] == -1);
    std::set<int> seen(l.begin() + 1, l.end());
    EXPECT(seen.size() == l.size() - 1 && *seen.begin() >= 0 && *seen.rbegin() < (int)(1049 * 0.98));
    EXPECT(l == sampledTrajectoryList(1049, 0.05, 9, nullptr, 0) && l != sampledTrajectoryList(1049, 0.05, 10, nullptr, 0));
    l = sampledTrajectoryList(200, 0.99, 1, top, 3);
    EXPECT((int)l.size() == 1 + 198 + 3 && l[1] == 0 && l[198] == 197 && l[199] == 7);
    l = sampledTrajectoryList(16384, 0.5, 1, top, 3);  // cut at the replay limit
    EXPECT((int)l.size() == REPLAY_N_MAX);
    l = sampledTrajectoryList(1, 0.5, 1, nullptr, 0);  // an empty pool
    EXPECT((l == std::vector<int>{ -1 }));
    l = sampledTrajectoryList(3, 0.9, 1, nullptr, 0);  // a draw larger than the pool takes the pool
    EXPECT(l.size() == 3 && l[0] == -1);
    EXPECT(sampledCount(-1.0, 100) == 0 && sampledCount(2.0, 100) == 100 && sampledCount(0.5, 0) == 0);
  }
  std::printf("replay host checks ok\n");
  return 0;
}
