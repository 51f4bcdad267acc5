/**
 * compute_feedback_host.cpp — TEST CODE: the name-keyed C++ controller's DDP feedback methods (include/mppi_amd/controllers.hpp)
 * on the cartpole, host-only C++ over the C ABI.  Prints (float64 sums over the float32 gains in order):
 *   points <entries> <sum at two fixed points cycled over the horizon>
 *   trajectory <entries> <sum along the last computeControl's result> <sum at the sequences read back>
 * tests/test_feedback_gpu.py forms the same sums from the Python methods on a controller set up the same way;
 * tests/probes/compute_feedback_templated.hip prints the same lines from the templated controller.
 */
#include <cstdio>
#include <vector>

#include "mppi_amd/controllers.hpp"

static double checksum(const std::vector<float>& G)
{
  double s = 0.0;
  for (float v : G)
    s += (double)v;
  return s;
}

int main()
{
  try
  {
    const int T = 10;
    mppi_amd::VanillaMPPIController controller("cartpole", 64, T, 0.02f, 1, 0.25f, 0.0f);
    controller.setDynamicsParams(mppi_cartpole_dynamics_params{ 1.5f, 0.3f, 0.7f });
    controller.setControlRanges({ -5.0f, 5.0f });
    controller.setSamplingParams({ 5.0f });
    const float Q[16] = { 5, 0, 0, 0, 0, 1, 0, 0, 0, 0, 20, 0, 0, 0, 0, 2 };
    const float R[1] = { 0.5f };
    const float Qf[16] = { 3, 0, 0, 0, 0, 3, 0, 0, 0, 0, 3, 0, 0, 0, 0, 3 };
    controller.setFeedbackParams(Q, R, Qf);
    const float px[2][4] = { { 0.3f, -0.4f, 0.7f, 1.5f }, { -1.0f, 0.2f, 2.9f, -2.0f } };
    const float pu[2] = { 2.0f, -4.0f };
    std::vector<float> x, u;
    for (int t = 0; t < T; t++)
    {
      x.insert(x.end(), px[t % 2], px[t % 2] + 4);
      u.push_back(pu[t % 2]);
    }
    std::vector<float> G = controller.computeFeedbackAt(x.data(), u.data());
    printf("points %zu %.17g\n", G.size(), checksum(G));
    controller.computeControl({ 0.0f, 0.0f, 0.5f, 0.0f }, 1);
    G = controller.computeFeedback();
    const std::vector<float> x_seq = controller.getTargetStateSeq(), u_seq = controller.getControlSeq();
    const std::vector<float> G_p = controller.computeFeedbackAt(x_seq.data(), u_seq.data());
    printf("trajectory %zu %.17g %.17g\n", G.size(), checksum(G), checksum(G_p));
    return 0;
  }
  catch (const std::exception& e)
  {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}
