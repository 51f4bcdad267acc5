// evaluateControls / warmStart of the two C++ host classes on Cartpole (tests/test_evaluate_cpp.py): what the templated
// controller and the named one return equals, bit for bit, what the C ABI returns on the same handle, and the installed sequence
// is the candidate the choice rule names.
#include <cstdio>
#include <cstring>
#include <vector>

#include <mppi/controllers/MPPI/mppi_controller.cuh>
#include <mppi/cost_functions/cartpole/cartpole_quadratic_cost.cuh>
#include <mppi/dynamics/cartpole/cartpole_dynamics.cuh>
#include <mppi/feedback_controllers/DDP/ddp.cuh>

#include "mppi_amd/controllers.hpp"
#include "mppi_amd/engine/evaluate_host.hpp"

constexpr int HORIZON = 9, ROLLOUTS = 200, N = 3;
using Sampler = mppi::sampling_distributions::GaussianDistribution<CartpoleDynamics::DYN_PARAMS_T>;
using Feedback = DDPFeedback<CartpoleDynamics, HORIZON>;
using CartpoleMPPI = VanillaMPPIController<CartpoleDynamics, CartpoleQuadraticCost, Feedback, HORIZON, ROLLOUTS, Sampler>;

#define EXPECT(cond)                                                \
  do                                                                \
  {                                                                 \
    if (!(cond))                                                    \
    {                                                               \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                     \
    }                                                               \
  } while (0)

static bool sameBits(const float* a, const float* b, size_t n)
{
  return std::memcmp(a, b, n * sizeof(float)) == 0;
}

int main()
{
  const float level[N] = { 0.0f, 3.0f, -3.0f };
  std::vector<float> rows((size_t)N * HORIZON);  // [N][T][C], C = 1
  for (int i = 0; i < N; i++)
    for (int t = 0; t < HORIZON; t++)
      rows[(size_t)i * HORIZON + t] = level[i] * (float)(t + 1) / (float)HORIZON;
  const float x0[4] = { 0.0f, 0.0f, 0.3f, 0.0f };

  /* ---- the templated controller ---- */
  {
    CartpoleDynamics model(1.0f, 1.0f, 1.0f);
    CartpoleQuadraticCost cost;
    auto sampler_params = Sampler::SAMPLING_PARAMS_T();
    sampler_params.std_dev[0] = 5.0f;
    Sampler sampler(sampler_params);
    Feedback fb(&model, 0.02f);
    CartpoleMPPI controller(&model, &cost, &fb, &sampler, 0.02f, 1, 200.0f, 0.0f);
    CartpoleDynamics::state_array x = CartpoleDynamics::state_array::Zero();
    std::copy(x0, x0 + 4, x.data());
    std::vector<CartpoleMPPI::control_trajectory> cands(N, CartpoleMPPI::control_trajectory::Zero());
    for (int i = 0; i < N; i++)
      std::copy(rows.begin() + (size_t)i * HORIZON, rows.begin() + (size_t)(i + 1) * HORIZON, cands[i].data());
    std::vector<int> crash;
    const std::vector<float> costs = controller.evaluateControls(x, cands, &crash);  // (creates the handle: before any iteration)
    EXPECT(costs.size() == N && crash.size() == N);
    float abi_cost[N];
    int abi_crash[N];
    EXPECT(mppi_evaluate_controls(controller.handle(), x0, 1, rows.data(), N, abi_cost, abi_crash) == MPPI_OK);
    EXPECT(sameBits(costs.data(), abi_cost, N) && std::memcmp(crash.data(), abi_crash, sizeof(abi_crash)) == 0);
    EXPECT(costs[0] != costs[1] && costs[1] != costs[2]);
    const std::vector<float> per_row = controller.evaluateControls(std::vector<CartpoleDynamics::state_array>(N, x), cands);
    EXPECT(sameBits(per_row.data(), costs.data(), N));
    std::vector<float> all;
    const int chosen = controller.warmStart(x, cands, 0.0f, &all);
    EXPECT(all.size() == N + 1 && sameBits(all.data() + 1, costs.data(), N));
    EXPECT(chosen == mppi::evaluate::warmStartChoice(all.data(), N, 0.0f));
    if (chosen >= 0)
    {
      const CartpoleMPPI::control_trajectory u = controller.getControlSeq();
      EXPECT(sameBits(u.data(), rows.data() + (size_t)chosen * HORIZON, HORIZON));
    }
    EXPECT(controller.warmStart(x, cands, 1e30f) == -1);
    std::printf("templated chosen %d\n", chosen);
  }
  /* ---- the named controller ---- */
  {
    mppi_amd::VanillaMPPIController controller("cartpole", ROLLOUTS, HORIZON, 0.02f, 1, 200.0f, 0.0f);
    const std::vector<float> x(x0, x0 + 4);
    std::vector<int> crash;
    const std::vector<float> costs = controller.evaluateControls(x, rows, &crash);
    float abi_cost[N];
    int abi_crash[N];
    EXPECT(mppi_evaluate_controls(controller.handle(), x0, 1, rows.data(), N, abi_cost, abi_crash) == MPPI_OK);
    EXPECT(costs.size() == N && sameBits(costs.data(), abi_cost, N) && std::memcmp(crash.data(), abi_crash, sizeof(abi_crash)) == 0);
    std::vector<float> all;
    const int chosen = controller.warmStart(x, rows, 0.0f, &all);
    EXPECT(all.size() == N + 1 && sameBits(all.data() + 1, costs.data(), N));
    EXPECT(chosen == mppi::evaluate::warmStartChoice(all.data(), N, 0.0f));
    if (chosen >= 0)
      EXPECT(sameBits(controller.getControlSeq().data(), rows.data() + (size_t)chosen * HORIZON, HORIZON));
    bool refused = false;
    try
    {
      controller.warmStart(x, rows, -1.0f);
    }
    catch (const mppi_amd::Error& e)
    {
      refused = e.status == MPPI_ERR_INVALID_ARG;
    }
    EXPECT(refused);
    std::printf("named chosen %d\n", chosen);
  }
  std::printf("evaluate controls cpp ok\n");
  return 0;
}
