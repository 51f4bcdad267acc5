/**
 * The reference's quadrotor hover loop (tests/controllers/vanilla_mppi_test.cu:160-312, Quadrotor_VanillaMPPI.HoverTest) set up
 * the reference's way — plugin objects + the TEMPLATED controller class — on this engine, like examples/templated_cartpole.hip:
 * K = 2048, T = 150, dt = 0.01, lambda = 4, alpha = 0.9, std_dev 0.5 / 0.5 / 0.5 / 2.0, goal 1 m above the start, the initial
 * control sequence at hover thrust; the plant is the model's own step.
 *
 * Build:  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I<repo>/include examples/templated_quadrotor.hip \
 *               -L<repo>/mppi-generic_amd/lib -lmppi_amd -Wl,-rpath,<repo>/mppi-generic_amd/lib -o templated_quadrotor
 * Run:    ./templated_quadrotor [steps] [lanes per rollout]    lanes = dynamics_rollout_dim_.y: 1 (default) or 4 — dim3(64, 4, 1),
 *         the four-lane shape the templated classes instantiate for every model (the reference's dim3(32, 4, 1) for this test
 *         is a shape of the registration unit, examples/quadrotor_model/).  Prints the state every 500 steps and how many steps ended outside the 0.15 m
 *         ball around the goal (the reference accepts fewer than 10 %).
 */
#include <mppi/controllers/MPPI/mppi_controller.cuh>
#include <mppi/cost_functions/quadrotor/quadrotor_quadratic_cost.cuh>
#include <mppi/dynamics/quadrotor/quadrotor_dynamics.cuh>
#include <mppi/feedback_controllers/DDP/ddp.cuh>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>

using Sampler = mppi::sampling_distributions::GaussianDistribution<QuadrotorDynamics::DYN_PARAMS_T>;
constexpr int HORIZON = 150;
constexpr int ROLLOUTS = 2048;
using Feedback = DDPFeedback<QuadrotorDynamics, HORIZON>;
using QuadrotorMPPI = VanillaMPPIController<QuadrotorDynamics, QuadrotorQuadraticCost, Feedback, HORIZON, ROLLOUTS, Sampler>;

int main(int argc, char** argv)
{
  const int steps = argc > 1 ? atoi(argv[1]) : 3000;
  const int lanes = argc > 2 ? atoi(argv[2]) : 1;

  QuadrotorDynamics model;  // thrust in [0, 36] N, zero control = hover thrust
  QuadrotorQuadraticCost cost;
  QuadrotorQuadraticCostParams cost_params;
  cost_params.x_goal()[2] = 1;
  cost_params.x_coeff = 400;
  cost_params.v_coeff = 150;
  cost_params.roll_coeff = 15;
  cost_params.pitch_coeff = 15;
  cost_params.yaw_coeff = 15;
  cost_params.w_coeff = 5;
  cost.setParams(cost_params);

  auto sampler_params = Sampler::SAMPLING_PARAMS_T();
  for (int i = 0; i < QuadrotorDynamics::CONTROL_DIM; i++)
    sampler_params.std_dev[i] = i == 3 ? 2.0f : 0.5f;
  Sampler sampler(sampler_params);

  const float dt = 0.01f, lambda = 4.0f, alpha = 0.9f;
  const int max_iter = 1;
  Feedback fb_controller(&model, dt);

  QuadrotorMPPI::control_trajectory init_control = QuadrotorMPPI::control_trajectory::Zero();
  for (int t = 0; t < HORIZON; t++)
    init_control(3, t) = mppi::math::GRAVITY;

  QuadrotorMPPI controller(&model, &cost, &fb_controller, &sampler, dt, max_iter, lambda, alpha, HORIZON, init_control);
  auto controller_params = controller.getParams();
  controller_params.dynamics_rollout_dim_ = dim3(64, lanes, 1);
  controller_params.cost_rollout_dim_ = dim3(64, lanes, 1);
  controller.setParams(controller_params);

  QuadrotorDynamics::state_array x = model.getZeroState(), x_next = x, xdot = x;
  QuadrotorDynamics::output_array y = QuadrotorDynamics::output_array::Zero();

  int far_away = 0;
  const auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < steps; i++)
  {
    controller.computeControl(x, 1);
    QuadrotorDynamics::control_array u = controller.getControlSeq().block(0, 0, QuadrotorDynamics::CONTROL_DIM, 1);
    model.enforceConstraints(x, u);
    model.step(x, x_next, xdot, u, y, (float)i, dt);
    x = x_next;
    if (i % 500 == 0)
    {
      printf("t = %5.2f s   baseline cost %10.3f   ", i * dt, controller.getBaselineCost());
      model.printState(x.data());
    }
    controller.slideControlSequence(1);
    const float dz = x[2] - cost_params.x_goal()[2];
    if (std::sqrt(x[0] * x[0] + x[1] * x[1] + dz * dz) > 0.15f)
      far_away++;
  }
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  const float qn = std::sqrt(x[6] * x[6] + x[7] * x[7] + x[8] * x[8] + x[9] * x[9]);
  printf("%s: %d control steps in %.1f ms, %d outside the ball, height %.4f m, |q| %.6f\n", controller.getControllerName().c_str(),
         steps, ms, far_away, x[2], qn);
  return 0;
}
