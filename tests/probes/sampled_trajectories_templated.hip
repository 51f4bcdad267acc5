// The reference-named sampled-trajectory methods of the templated host classes on Cartpole (tests/test_replay_cpp.py): prints
// the first top-N index and cost from the class and from the C ABI on a second, identically seeded handle's own selection.
#include <cstdio>
#include <vector>

#include <mppi/controllers/MPPI/mppi_controller.cuh>
#include <mppi/cost_functions/cartpole/cartpole_quadratic_cost.cuh>
#include <mppi/dynamics/cartpole/cartpole_dynamics.cuh>
#include <mppi/feedback_controllers/DDP/ddp.cuh>

constexpr int HORIZON = 17, ROLLOUTS = 1049;
using Sampler = mppi::sampling_distributions::GaussianDistribution<CartpoleDynamics::DYN_PARAMS_T>;
using Feedback = DDPFeedback<CartpoleDynamics, HORIZON>;
using CartpoleMPPI = VanillaMPPIController<CartpoleDynamics, CartpoleQuadraticCost, Feedback, HORIZON, ROLLOUTS, Sampler>;

int main()
{
  CartpoleDynamics model(1.0f, 1.0f, 1.0f);
  CartpoleQuadraticCost cost;
  auto sampler_params = Sampler::SAMPLING_PARAMS_T();
  sampler_params.std_dev[0] = 5.0f;
  Sampler sampler(sampler_params);
  Feedback fb(&model, 0.02f);
  CartpoleMPPI controller(&model, &cost, &fb, &sampler, 0.02f, 1, 200.0f, 0.0f);
  controller.setTopNSampledControlTrajectories(7);
  controller.setPercentageSampledControlTrajectories(0.01f);
  CartpoleDynamics::state_array x = CartpoleDynamics::state_array::Zero();
  controller.computeControl(x, 1);
  controller.calculateSampledStateTrajectories();
  const std::vector<int>& rows = controller.getSampledTrajectoryIndices();
  const std::vector<float>& top = controller.getTopNCosts();
  const int n_rand = (int)(0.01f * ROLLOUTS);
  if ((int)rows.size() != 1 + n_rand + 7 || rows[0] != -1 || top.size() != 7)
  {
    printf("FAILED list: %zu rows\n", rows.size());
    return 1;
  }
  // the same selection through the C ABI, and all costs for the caller to sort
  int idx[7];
  float val[7];
  if (mppi_top_rollouts(controller.handle(), 0, 7, idx, val) != MPPI_OK)
  {
    printf("FAILED mppi_top_rollouts: %s\n", mppi_last_error(controller.handle()));
    return 1;
  }
  const std::vector<float> costs = controller.getSampledCostSeq();
  int best = 0;
  for (int k = 1; k < ROLLOUTS; k++)
    if (costs[k] < costs[best])
      best = k;
  printf("class %d %.9g abi %d %.9g scan %d %.9g\n", rows[1 + n_rand], top[0], idx[0], val[0], best, costs[best]);
  const size_t O = CartpoleDynamics::OUTPUT_DIM;
  printf("shapes %zu %zu %zu\n", controller.getSampledOutputTrajectories().size() / (rows.size() * HORIZON * O),
         controller.getSampledCostTrajectories().size() / (rows.size() * (HORIZON + 1)),
         controller.getSampledCrashStatusTrajectories().size() / (rows.size() * HORIZON));
  return 0;
}
