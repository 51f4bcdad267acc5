/**
 * compute_grad_templated.hip — TEST CODE: the templated controller's computeGrad(state, control, A, B) and computeGradTrajectory
 * (include/mppi_amd/controllers_templated.hpp) on the cartpole, written against the reference's include paths.  linearizeKernel is
 * instantiated in THIS translation unit, through the ModelT the class registers.  Prints what tests/probes/compute_grad_host.cpp
 * prints, in the same order of additions (float64 sums over the float32 entries, A then B, point after point):
 *   points <entries of A> <entries of B> <sum at the two fixed points>
 *   trajectory <entries of A> <entries of B> <sum along the last computeControl's result> <sum at the sequences read back>
 * tests/test_linearize_gpu.py compares the first sum with Python's and the last two with each other.
 */
#include <mppi/instantiations/cartpole_mppi/cartpole_mppi.cuh>

#include <cstdio>
#include <vector>

using Sampler = mppi::sampling_distributions::GaussianDistribution<CartpoleDynamics::DYN_PARAMS_T>;
const int HORIZON = 10;
const int ROLLOUTS = 64;
using Feedback = DDPFeedback<CartpoleDynamics, HORIZON>;
using CartpoleMPPI = VanillaMPPIController<CartpoleDynamics, CartpoleQuadraticCost, Feedback, HORIZON, ROLLOUTS>;
constexpr int S = CartpoleDynamics::STATE_DIM, C = CartpoleDynamics::CONTROL_DIM;

int main()
{
  try
  {
    CartpoleDynamics model(1.5f, 0.3f, 0.7f);
    model.control_rngs_->x = -5;
    model.control_rngs_->y = 5;
    CartpoleQuadraticCost cost;
    auto sampler_params = Sampler::SAMPLING_PARAMS_T();
    sampler_params.std_dev[0] = 5.0f;
    Sampler sampler(sampler_params);
    const float dt = 0.02f;
    Feedback fb_controller(&model, dt);
    CartpoleMPPI controller(&model, &cost, &fb_controller, &sampler, dt, 1, 0.25f, 0.0f);

    const float points[2][S + C] = { { 0.3f, -0.4f, 0.7f, 1.5f, 2.0f }, { -1.0f, 0.2f, 2.9f, -2.0f, -4.0f } };
    float A[S * S], B[S * C];
    // the sum of one point's entries joins the running sum entry by entry: the order a flat [n][S][S] | [n][S][C] pass takes
    std::vector<float> all_a, all_b;
    auto at = [&](const float* x, const float* u) {
      CartpoleMPPI::state_array xs = CartpoleMPPI::state_array::Zero();
      CartpoleMPPI::control_array us = CartpoleMPPI::control_array::Zero();
      for (int i = 0; i < S; i++)
        xs[i] = x[i];
      for (int i = 0; i < C; i++)
        us[i] = u[i];
      if (!controller.computeGrad(xs, us, A, B))
        throw std::runtime_error("the templated cartpole reports no computeGrad");
      all_a.insert(all_a.end(), A, A + S * S);
      all_b.insert(all_b.end(), B, B + S * C);
    };
    auto total = [](const std::vector<float>& a, const std::vector<float>& b) {
      double s = 0.0;
      for (float v : a)
        s += (double)v;
      for (float v : b)
        s += (double)v;
      return s;
    };
    for (const auto& p : points)
      at(p, p + S);
    printf("points %zu %zu %.17g\n", all_a.size(), all_b.size(), total(all_a, all_b));

    CartpoleMPPI::state_array x0 = CartpoleMPPI::state_array::Zero();
    x0[2] = 0.5f;
    controller.computeControl(x0, 1);
    std::vector<float> traj_a, traj_b;
    controller.computeGradTrajectory(traj_a, traj_b);
    const auto x_seq = controller.getTargetStateSeq();
    const auto u_seq = controller.getControlSeq();
    all_a.clear();
    all_b.clear();
    for (int t = 0; t < HORIZON; t++)
      at(x_seq.data() + t * S, u_seq.data() + t * C);
    printf("trajectory %zu %zu %.17g %.17g\n", traj_a.size(), traj_b.size(), total(traj_a, traj_b), total(all_a, all_b));
    return 0;
  }
  catch (const std::exception& e)
  {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}
