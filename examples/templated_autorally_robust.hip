/**
 * The reference's AutoRally Robust MPPI set-up through the TEMPLATED controllers: NeuralNetModel<7,2,3> + ARRobustCost +
 * DDPFeedback, first with VanillaMPPIController, then with RobustMPPIController, on a synthetic network and a synthetic
 * four-channel track map, both built in code.  The network (6-32-32-4, 1412 parameters) and the map (22 rows x 28 columns of
 * 0.1 m texels; boundary constraint in bands of 0 / 0.6 / 1, track position, speed map, heading) reach the engine as the
 * "dynamics_weights" and "costmap" blobs of each controller's handle; the map's transform is in the cost's parameters.
 *
 * K = 1024, T = 20, dt = 0.1, lambda = 20, alpha = 0, std_dev 0.3 / 0.3, control cost 0.2 / 0.1, steering in [-0.99, 0.99],
 * throttle in [-0.99, 0.65]; the vehicle starts at (-12.05, 5.05) at 4 m/s.  The plant is the model's own prediction: the
 * next state is the second column of the controller's state trajectory.
 *
 * Build:  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I<repo>/include examples/templated_autorally_robust.hip \
 *               -L<repo>/mppi-generic_amd/lib -lmppi_amd -Wl,-rpath,<repo>/mppi-generic_amd/lib -o templated_autorally_robust
 * Run:    ./templated_autorally_robust [steps]    (default 5).  Prints, for either controller, the control sequence and the
 *         baseline of the FIRST computeControl, then the state after the closed-loop steps.
 */
#include <mppi/controllers/MPPI/mppi_controller.cuh>
#include <mppi/controllers/R-MPPI/robust_mppi_controller.cuh>
#include <mppi/cost_functions/autorally/ar_robust_cost.cuh>
#include <mppi/dynamics/autorally/ar_nn_model.cuh>
#include <mppi/feedback_controllers/DDP/ddp.cuh>

#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <vector>

using Dyn = NeuralNetModel<7, 2, 3>;
constexpr int HORIZON = 20;
constexpr int ROLLOUTS = 1024;
using Feedback = DDPFeedback<Dyn, HORIZON>;
using Sampler = mppi::sampling_distributions::GaussianDistribution<Dyn::DYN_PARAMS_T>;
using Vanilla = VanillaMPPIController<Dyn, ARRobustCost, Feedback, HORIZON, ROLLOUTS, Sampler>;
using Robust = RobustMPPIController<Dyn, ARRobustCost, Feedback, HORIZON, ROLLOUTS, Sampler>;

constexpr int MAP_WIDTH = 28, MAP_HEIGHT = 22;
constexpr double MAP_X_MIN = -12.5, MAP_X_MAX = -9.7, MAP_Y_MIN = 3.8, MAP_Y_MAX = 6.0;
constexpr int NUM_WEIGHTS = 6 * 32 + 32 + 32 * 32 + 32 + 32 * 4 + 4;

/** [W1 | b1 | W2 | b2 | W3 | b3]: multiples of 0.0003 in [-0.3, 0.3] from an integer sequence */
static std::vector<float> syntheticNetwork()
{
  std::vector<float> w(NUM_WEIGHTS);
  for (unsigned i = 0; i < (unsigned)NUM_WEIGHTS; i++)
    w[i] = (float)((int)((i * 7919u + 13u) % 2001u) - 1000) * 0.0003f;
  return w;
}

/** texels [row][column][4] */
static std::vector<float> syntheticMap()
{
  std::vector<float> t((size_t)MAP_WIDTH * MAP_HEIGHT * 4);
  for (int r = 0; r < MAP_HEIGHT; r++)
    for (int c = 0; c < MAP_WIDTH; c++)
    {
      const int band = c + 3 * (r >= 16);
      float* texel = &t[((size_t)r * MAP_WIDTH + c) * 4];
      texel[0] = band >= 20 ? 1.0f : band >= 16 ? 0.6f : 0.0f;  // boundary constraint
      texel[1] = (float)(0.05 * c + 0.01 * r);                   // track position
      texel[2] = (float)(3.0 + 0.1 * c - 0.05 * r);              // speed map
      texel[3] = (float)(0.3 - 0.02 * c + 0.01 * r);             // heading
    }
  return t;
}

template <class CONTROLLER_T>
static int run(CONTROLLER_T& controller, const char* tag, int steps)
{
  const std::vector<float> weights = syntheticNetwork(), map = syntheticMap();
  const int weight_dims[1] = { NUM_WEIGHTS }, map_dims[3] = { MAP_HEIGHT, MAP_WIDTH, 4 };
  if (mppi_set_model_blob(controller.handle(), "dynamics_weights", weights.data(), weights.size(), weight_dims, 1) != MPPI_OK ||
      mppi_set_model_blob(controller.handle(), "costmap", map.data(), map.size(), map_dims, 3) != MPPI_OK)
  {
    fprintf(stderr, "%s: setting the network or the map failed: %s\n", tag, mppi_last_error(controller.handle()));
    return 2;
  }
  Dyn::state_array x = Dyn::state_array::Zero();
  x[0] = -12.05f;
  x[1] = 5.05f;
  x[4] = 4.0f;
  x[5] = -0.05f;
  for (int i = 0; i < steps; i++)
  {
    if constexpr (std::is_same<CONTROLLER_T, Robust>::value)
      controller.updateImportanceSamplingControl(x, 1);
    controller.computeControl(x, 1);
    if (i == 0)
    {
      const auto u = controller.getControlSeq();
      for (int t = 0; t < HORIZON; t++)
        printf("%s u[%d] = %.9g %.9g\n", tag, t, u(0, t), u(1, t));
      printf("%s baseline = %.9g\n", tag, controller.getBaselineCost());
    }
    x = controller.getTargetStateSeq().col(1);
    controller.slideControlSequence(1);
  }
  printf("%s: after %d steps at %.4f %.4f, yaw %.4f, speed %.4f\n", controller.getControllerName().c_str(), steps, x[0], x[1], x[2],
         x[4]);
  return 0;
}

int main(int argc, char** argv)
{
  const int steps = argc > 1 ? atoi(argv[1]) : 5;
  const float dt = 0.1f, lambda = 20.0f, alpha = 0.0f;
  const int max_iter = 1;

  Dyn model;
  const float2 ranges[2] = { make_float2(-0.99f, 0.99f), make_float2(-0.99f, 0.65f) };
  model.setControlRanges(ranges);

  ARRobustCost cost;
  ARRobustCostParams cost_params;
  cost_params.boundary_threshold = 0.5f;
  cost_params.track_slop = 1.0f;
  cost_params.heading_coeff = 20;
  cost_params.slip_coeff = 10;
  cost_params.crash_coeff = 10000;
  cost_params.max_slip_ang = 0.03f;
  // world -> texture, the transform loadTrackData builds from the map's bounds
  cost_params.r_c1[0] = (float)(1.0 / (MAP_X_MAX - MAP_X_MIN));
  cost_params.r_c2[1] = (float)(1.0 / (MAP_Y_MAX - MAP_Y_MIN));
  cost_params.trs[0] = (float)(-MAP_X_MIN / (MAP_X_MAX - MAP_X_MIN));
  cost_params.trs[1] = (float)(-MAP_Y_MIN / (MAP_Y_MAX - MAP_Y_MIN));
  cost.setParams(cost_params);

  auto sampler_params = Sampler::SAMPLING_PARAMS_T();
  sampler_params.std_dev[0] = sampler_params.std_dev[1] = 0.3f;
  sampler_params.control_cost_coeff[0] = 0.2f;
  sampler_params.control_cost_coeff[1] = 0.1f;
  Sampler sampler(sampler_params);

  Feedback fb_controller(&model, dt);
  // gains[t][state][control]: the lateral velocity and the yaw rate steer, the speed error throttles
  std::vector<float> gains((size_t)HORIZON * Dyn::STATE_DIM * Dyn::CONTROL_DIM, 0.0f);
  for (int t = 0; t < HORIZON; t++)
  {
    gains[((size_t)t * Dyn::STATE_DIM + 5) * Dyn::CONTROL_DIM + 0] = -0.25f;
    gains[((size_t)t * Dyn::STATE_DIM + 6) * Dyn::CONTROL_DIM + 0] = 0.125f;
    gains[((size_t)t * Dyn::STATE_DIM + 4) * Dyn::CONTROL_DIM + 1] = -0.5f;
  }
  fb_controller.setFeedbackGains(gains);

  Vanilla vanilla(&model, &cost, &fb_controller, &sampler, dt, max_iter, lambda, alpha);
  int rc = run(vanilla, "vanilla", steps);
  if (rc)
    return rc;
  const float value_function_threshold = 1000.0f;
  Robust robust(&model, &cost, &fb_controller, &sampler, dt, max_iter, lambda, alpha, value_function_threshold);
  return run(robust, "robust", steps);
}
