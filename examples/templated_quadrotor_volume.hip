/**
 * A quadrotor flies from one side of a pillar to a goal behind it: QuadrotorDynamics + QuadrotorVolumeCost through the TEMPLATED
 * Vanilla controller, set up the reference's way like examples/templated_quadrotor.hip.  The clearance volume holds
 * max(0, 1 - distance / 1.5 m) to a vertical pillar at (2, 0), 16 x 12 x 6 cells of 0.5 m over x in [-2, 6), y in [-3, 3),
 * z in [0, 3); it reaches the cost's ThreeDTextureHelper as the "cost_volume" / "cost_volume_transform" blobs of the controller's
 * engine handle.  The cost is this project's own (the reference has no volume cost); the helper is the reference's
 * ThreeDTextureHelper, host formula.
 *
 * K = 256, T = 40, dt = 0.02, lambda = 5, alpha = 0, std_dev 0.5 / 0.5 / 0.5 / 2.0, control cost 1.
 *
 * Build:  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I<repo>/include examples/templated_quadrotor_volume.hip \
 *               -L<repo>/mppi-generic_amd/lib -lmppi_amd -Wl,-rpath,<repo>/mppi-generic_amd/lib -o templated_quadrotor_volume
 * Run:    ./templated_quadrotor_volume [steps]    (default 200).  Prints the first control sequence, then the closest approach to
 *         the pillar's axis and the final position.
 */
#include <mppi/controllers/MPPI/mppi_controller.cuh>
#include <mppi/cost_functions/quadrotor/quadrotor_volume_cost.cuh>
#include <mppi/dynamics/quadrotor/quadrotor_dynamics.cuh>
#include <mppi/feedback_controllers/DDP/ddp.cuh>
#include <mppi/utils/texture_helpers/three_d_texture_helper.cuh>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

using Sampler = mppi::sampling_distributions::GaussianDistribution<QuadrotorDynamics::DYN_PARAMS_T>;
constexpr int HORIZON = 40;
constexpr int ROLLOUTS = 256;
using Feedback = DDPFeedback<QuadrotorDynamics, HORIZON>;
using QuadrotorMPPI = VanillaMPPIController<QuadrotorDynamics, QuadrotorVolumeCost, Feedback, HORIZON, ROLLOUTS, Sampler>;

constexpr int VOL_WIDTH = 16, VOL_HEIGHT = 12, VOL_DEPTH = 6;  // x in [-2, 6), y in [-3, 3), z in [0, 3)
constexpr float CELL = 0.5f, VOL_X0 = -2.0f, VOL_Y0 = -3.0f, VOL_Z0 = 0.0f;
constexpr float PILLAR_X = 2.0f, PILLAR_Y = 0.0f, PILLAR_REACH = 1.5f;

/** max(0, 1 - distance / PILLAR_REACH) to the pillar's axis at every cell centre, the same in every layer */
static std::vector<float> pillarVolume()
{
  std::vector<float> v((size_t)VOL_WIDTH * VOL_HEIGHT * VOL_DEPTH);
  for (int z = 0; z < VOL_DEPTH; z++)
    for (int r = 0; r < VOL_HEIGHT; r++)
      for (int c = 0; c < VOL_WIDTH; c++)
      {
        const float x = VOL_X0 + CELL * (c + 0.5f), y = VOL_Y0 + CELL * (r + 0.5f);
        const float dist = std::sqrt((x - PILLAR_X) * (x - PILLAR_X) + (y - PILLAR_Y) * (y - PILLAR_Y));
        v[((size_t)z * VOL_HEIGHT + r) * VOL_WIDTH + c] = std::max(0.0f, 1.0f - dist / PILLAR_REACH);
      }
  return v;
}

int main(int argc, char** argv)
{
  const int steps = argc > 1 ? atoi(argv[1]) : 200;

  QuadrotorDynamics model;
  QuadrotorVolumeCost cost;
  QuadrotorVolumeCostParams cost_params;
  cost_params.x_goal()[0] = 4.0f;
  cost_params.x_goal()[1] = 0.25f;
  cost_params.x_goal()[2] = 1.5f;
  cost_params.x_coeff = 40;
  cost_params.v_coeff = 15;
  cost_params.roll_coeff = 15;
  cost_params.pitch_coeff = 15;
  cost_params.yaw_coeff = 15;
  cost_params.w_coeff = 5;
  cost_params.volume_coeff = 200.0f;
  cost_params.crash_threshold = 0.6f;
  cost_params.crash_coeff = 1000.0f;
  cost.setParams(cost_params);

  auto sampler_params = Sampler::SAMPLING_PARAMS_T();
  for (int i = 0; i < QuadrotorDynamics::CONTROL_DIM; i++)
  {
    sampler_params.std_dev[i] = i == 3 ? 2.0f : 0.5f;
    sampler_params.control_cost_coeff[i] = 1.0f;
  }
  Sampler sampler(sampler_params);

  const float dt = 0.02f, lambda = 5.0f, alpha = 0.0f;
  const int max_iter = 1;
  Feedback fb_controller(&model, dt);

  QuadrotorMPPI::control_trajectory init_control = QuadrotorMPPI::control_trajectory::Zero();
  for (int t = 0; t < HORIZON; t++)
    init_control(3, t) = mppi::math::GRAVITY;

  QuadrotorMPPI controller(&model, &cost, &fb_controller, &sampler, dt, max_iter, lambda, alpha, HORIZON, init_control);

  const std::vector<float> volume = pillarVolume();
  const int dims[3] = { VOL_DEPTH, VOL_HEIGHT, VOL_WIDTH };
  const float frame[15] = { VOL_X0, VOL_Y0, VOL_Z0, 1, 0, 0, 0, 1, 0, 0, 0, 1, CELL, CELL, CELL };
  if (mppi_set_model_blob(controller.handle(), "cost_volume_transform", frame, 15, nullptr, 0) != MPPI_OK ||
      mppi_set_model_blob(controller.handle(), "cost_volume", volume.data(), volume.size(), dims, 3) != MPPI_OK)
  {
    fprintf(stderr, "setting the clearance volume failed: %s\n", mppi_last_error(controller.handle()));
    return 2;
  }

  QuadrotorDynamics::state_array x = model.getZeroState(), x_next = x, xdot = x;
  x[0] = 0.0f;
  x[1] = 0.1f;
  x[2] = 1.5f;
  QuadrotorDynamics::output_array y = QuadrotorDynamics::output_array::Zero();

  float closest = 1e30f;
  for (int i = 0; i < steps; i++)
  {
    controller.computeControl(x, 1);
    if (i == 0)
    {
      const auto u = controller.getControlSeq();
      for (int t = 0; t < HORIZON; t++)
        printf("u[%d] = %.9g %.9g %.9g %.9g\n", t, u(0, t), u(1, t), u(2, t), u(3, t));
      printf("baseline = %.9g\n", controller.getBaselineCost());
    }
    QuadrotorDynamics::control_array u = controller.getControlSeq().block(0, 0, QuadrotorDynamics::CONTROL_DIM, 1);
    model.enforceConstraints(x, u);
    model.step(x, x_next, xdot, u, y, (float)i, dt);
    x = x_next;
    controller.slideControlSequence(1);
    closest = std::min(closest, std::sqrt((x[0] - PILLAR_X) * (x[0] - PILLAR_X) + (x[1] - PILLAR_Y) * (x[1] - PILLAR_Y)));
  }
  printf("%s: after %d steps at %.3f %.3f %.3f, closest approach to the pillar %.3f m\n", controller.getControllerName().c_str(), steps,
         x[0], x[1], x[2], closest);
  return 0;
}
