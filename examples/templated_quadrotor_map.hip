/**
 * A quadrotor flies a short course of three gates over a small synthetic track map: QuadrotorDynamics + QuadrotorMapCost through
 * the TEMPLATED Vanilla controller, set up the reference's way like examples/templated_quadrotor.hip.  The map holds the
 * distance to the course's centre line, (0, 0) -> (3, 0) -> (6, 2) -> (9, 2), in 0.5 m cells; it reaches the cost's
 * TwoDTextureHelper as the "costmap" / "costmap_transform" blobs of the controller's engine handle.  The waypoint is the next
 * gate: whenever the vehicle comes within gate_margin of it (distToWaypoint), updateWaypoint moves the cost on to the gate after
 * it and setParams hands the block to the controller, between two computeControl calls.  The plant is the model's own step.
 *
 * K = 256, T = 40, dt = 0.02, lambda = 5, alpha = 0, std_dev 0.5 / 0.5 / 0.5 / 2.0, control cost 1; gates 2 m wide at heading
 * pi / 2, gate_margin 0.75 m, desired speed 2 m/s, height / speed / heading coefficients 50 / 20 / 50.
 *
 * Build:  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I<repo>/include examples/templated_quadrotor_map.hip \
 *               -L<repo>/mppi-generic_amd/lib -lmppi_amd -Wl,-rpath,<repo>/mppi-generic_amd/lib -o templated_quadrotor_map
 * Run:    ./templated_quadrotor_map [steps]    (default 600).  Prints the step on which each gate was passed; returns 0 when all
 *         three were.
 */
#include <mppi/controllers/MPPI/mppi_controller.cuh>
#include <mppi/cost_functions/quadrotor/quadrotor_map_cost.cuh>
#include <mppi/dynamics/quadrotor/quadrotor_dynamics.cuh>
#include <mppi/feedback_controllers/DDP/ddp.cuh>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

using Sampler = mppi::sampling_distributions::GaussianDistribution<QuadrotorDynamics::DYN_PARAMS_T>;
constexpr int HORIZON = 40;
constexpr int ROLLOUTS = 256;
using Feedback = DDPFeedback<QuadrotorDynamics, HORIZON>;
using QuadrotorMPPI = VanillaMPPIController<QuadrotorDynamics, QuadrotorMapCost, Feedback, HORIZON, ROLLOUTS, Sampler>;

constexpr int NUM_GATES = 3;
constexpr int MAP_WIDTH = 26, MAP_HEIGHT = 16;  // x in [-2, 11), y in [-3, 5)
constexpr float CELL = 0.5f, MAP_X0 = -2.0f, MAP_Y0 = -3.0f;

/** distance [m] of every cell centre to the centre line of the course */
static std::vector<float> courseMap()
{
  const double line[4][2] = { { 0, 0 }, { 3, 0 }, { 6, 2 }, { 9, 2 } };
  std::vector<float> map((size_t)MAP_WIDTH * MAP_HEIGHT);
  for (int r = 0; r < MAP_HEIGHT; r++)
    for (int c = 0; c < MAP_WIDTH; c++)
    {
      const double x = MAP_X0 + CELL * (c + 0.5), y = MAP_Y0 + CELL * (r + 0.5);
      double best = 1e30;
      for (int i = 0; i < 3; i++)
      {
        const double ax = line[i][0], ay = line[i][1], bx = line[i + 1][0] - ax, by = line[i + 1][1] - ay;
        const double t = std::min(1.0, std::max(0.0, ((x - ax) * bx + (y - ay) * by) / (bx * bx + by * by)));
        best = std::min(best, std::hypot(x - ax - t * bx, y - ay - t * by));
      }
      map[(size_t)r * MAP_WIDTH + c] = (float)best;
    }
  return map;
}

int main(int argc, char** argv)
{
  const int steps = argc > 1 ? atoi(argv[1]) : 600;
  const float half_pi = (float)M_PI_2;
  const float gates[NUM_GATES][4] = { { 3.0f, 0.0f, 1.2f, half_pi }, { 6.0f, 2.0f, 1.5f, half_pi }, { 9.0f, 2.0f, 1.0f, half_pi } };

  QuadrotorDynamics model;
  QuadrotorMapCost cost;
  QuadrotorMapCostParams cost_params;
  cost_params.gate_width = 1.0f;
  cost_params.gate_margin = 0.75f;
  cost_params.desired_speed = 2.0f;
  cost_params.height_coeff = 50;
  cost_params.speed_coeff = 20;
  cost_params.heading_coeff = 50;
  cost_params.updateWaypoint(0.0f, 0.0f, 1.0f, half_pi);  // the start, so that the first gate has a previous waypoint
  cost_params.updateWaypoint(gates[0][0], gates[0][1], gates[0][2], gates[0][3]);
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

  // the track map and its frame: origin of the map in the world, no rotation, metres per cell
  const std::vector<float> map = courseMap();
  const int dims[2] = { MAP_HEIGHT, MAP_WIDTH };
  const float frame[15] = { MAP_X0, MAP_Y0, 0.0f, 1, 0, 0, 0, 1, 0, 0, 0, 1, CELL, CELL, 1.0f };
  if (mppi_set_model_blob(controller.handle(), "costmap_transform", frame, 15, nullptr, 0) != MPPI_OK ||
      mppi_set_model_blob(controller.handle(), "costmap", map.data(), map.size(), dims, 2) != MPPI_OK)
  {
    fprintf(stderr, "setting the track map failed: %s\n", mppi_last_error(controller.handle()));
    return 2;
  }

  QuadrotorDynamics::state_array x = model.getZeroState(), x_next = x, xdot = x;
  x[2] = 1.0f;
  QuadrotorDynamics::output_array y = QuadrotorDynamics::output_array::Zero();

  int gate = 0;
  const auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < steps && gate < NUM_GATES; i++)
  {
    controller.computeControl(x, 1);
    QuadrotorDynamics::control_array u = controller.getControlSeq().block(0, 0, QuadrotorDynamics::CONTROL_DIM, 1);
    model.enforceConstraints(x, u);
    model.step(x, x_next, xdot, u, y, (float)i, dt);
    x = x_next;
    controller.slideControlSequence(1);
    if (cost.distToWaypoint(x.data(), cost_params.curr_waypoint) < cost_params.gate_margin)
    {
      printf("gate %d passed at step %d   position %.3f %.3f %.3f   baseline cost %.2f\n", gate + 1, i + 1, x[0], x[1], x[2],
             controller.getBaselineCost());
      gate++;
      if (gate < NUM_GATES)
      {
        cost_params.updateWaypoint(gates[gate][0], gates[gate][1], gates[gate][2], gates[gate][3]);
        cost.setParams(cost_params);  // the controller carries the block to the engine with the next computeControl
      }
    }
  }
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  printf("%s: %d of %d gates passed in %.1f ms, final position %.3f %.3f %.3f\n", controller.getControllerName().c_str(), gate,
         NUM_GATES, ms, x[0], x[1], x[2]);
  return gate == NUM_GATES ? 0 : 1;
}
