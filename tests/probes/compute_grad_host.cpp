/**
 * compute_grad_host.cpp — TEST CODE: the name-keyed C++ controller's computeGrad accessors (include/mppi_amd/controllers.hpp) on
 * the cartpole, host-only C++ over the C ABI.  Prints (float64 sums over the float32 entries in order, A then B):
 *   points <entries of A> <entries of B> <sum at two fixed points>
 *   trajectory <entries of A> <entries of B> <sum along the last computeControl's result> <sum at the sequences read back>
 * tests/test_linearize_gpu.py forms the same sums from the Python methods on a controller set up the same way;
 * tests/probes/compute_grad_templated.hip prints the same lines from the templated controller.
 */
#include <cstdio>
#include <vector>

#include "mppi_amd/controllers.hpp"

static double checksum(const std::vector<float>& A, const std::vector<float>& B)
{
  double s = 0.0;
  for (float v : A)
    s += (double)v;
  for (float v : B)
    s += (double)v;
  return s;
}

int main()
{
  try
  {
    mppi_amd::VanillaMPPIController controller("cartpole", 64, 10, 0.02f, 1, 0.25f, 0.0f);
    controller.setDynamicsParams(mppi_cartpole_dynamics_params{ 1.5f, 0.3f, 0.7f });
    controller.setControlRanges({ -5.0f, 5.0f });
    controller.setSamplingParams({ 5.0f });
    if (!controller.hasComputeGrad())
    {
      fprintf(stderr, "cartpole reports no computeGrad\n");
      return 1;
    }
    const float x[8] = { 0.3f, -0.4f, 0.7f, 1.5f, -1.0f, 0.2f, 2.9f, -2.0f };
    const float u[2] = { 2.0f, -4.0f };
    std::vector<float> A, B;
    controller.computeGrad(x, u, 2, A, B);
    printf("points %zu %zu %.17g\n", A.size(), B.size(), checksum(A, B));
    controller.computeControl({ 0.0f, 0.0f, 0.5f, 0.0f }, 1);
    controller.computeGradTrajectory(A, B);
    const std::vector<float> x_seq = controller.getTargetStateSeq(), u_seq = controller.getControlSeq();
    std::vector<float> A_p, B_p;
    controller.computeGrad(x_seq.data(), u_seq.data(), 10, A_p, B_p);
    printf("trajectory %zu %zu %.17g %.17g\n", A.size(), B.size(), checksum(A, B), checksum(A_p, B_p));
    return 0;
  }
  catch (const std::exception& e)
  {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}
