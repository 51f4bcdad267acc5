/**
 * log-MPPI on the reference's templated host surface: VanillaMPPIController with NLNDistribution as its SAMPLING_T
 * (the reference: include/mppi/sampling_distributions/nln/nln.cuh handed to any controller template).
 *
 * Written against the reference's include paths and class names, like examples/templated_cartpole.hip; the one line that
 * differs from the Gaussian example is the Sampler alias and the sixth template argument of the controller.
 *
 * Build:  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I<repo>/include examples/templated_cartpole_nln.hip \
 *               -L<repo>/mppi-generic_amd/lib -lmppi_amd -Wl,-rpath,<repo>/mppi-generic_amd/lib -o templated_cartpole_nln
 * Run:    ./templated_cartpole_nln [steps]    one computeControl from a fixed state prints the optimal control sequence
 *         ("u[t] = ..."), then a closed loop of `steps` control steps (default 200) prints the final pole angle
 */
#include <mppi/instantiations/cartpole_mppi/cartpole_mppi.cuh>
#include <mppi/sampling_distributions/nln/nln.cuh>

#include <cstdio>
#include <cstdlib>

using Sampler = mppi::sampling_distributions::NLNDistribution<CartpoleDynamics::DYN_PARAMS_T>;
constexpr int HORIZON = 30;
constexpr int ROLLOUTS = 1024;
using Feedback = DDPFeedback<CartpoleDynamics, HORIZON>;
using CartpoleLogMPPI = VanillaMPPIController<CartpoleDynamics, CartpoleQuadraticCost, Feedback, HORIZON, ROLLOUTS, Sampler>;

int main(int argc, char** argv)
{
  const int steps = argc > 1 ? atoi(argv[1]) : 200;

  CartpoleDynamics model(1.0f, 1.0f, 1.0f);  // cart mass, pole mass, pole length
  model.control_rngs_->x = -5;
  model.control_rngs_->y = 5;

  CartpoleQuadraticCost cost;
  CartpoleQuadraticCostParams cost_params;
  cost_params.cart_position_coeff = 50;
  cost_params.pole_angle_coeff = 200;
  cost_params.cart_velocity_coeff = 10;
  cost_params.pole_angular_velocity_coeff = 1;
  cost_params.control_cost_coeff[0] = 0;
  cost_params.terminal_cost_coeff = 0;
  cost_params.desired_terminal_state[0] = 20;
  cost_params.desired_terminal_state[1] = 0;
  cost_params.desired_terminal_state[2] = M_PI;
  cost_params.desired_terminal_state[3] = 0;
  cost.setParams(cost_params);

  // the normal factor is scaled by std_dev as in the Gaussian sampler; the log-normal factor is exp(std_dev * z'), so a
  // std_dev below 1 keeps the tail of the product moderate
  auto sampler_params = Sampler::SAMPLING_PARAMS_T();
  for (int i = 0; i < CartpoleDynamics::CONTROL_DIM; i++)
    sampler_params.std_dev[i] = 0.8f;
  Sampler sampler(sampler_params);

  const float dt = 0.02f, lambda = 20.0f, alpha = 0.0f;
  const int max_iter = 1;
  Feedback fb_controller(&model, dt);

  CartpoleLogMPPI controller(&model, &cost, &fb_controller, &sampler, dt, max_iter, lambda, alpha);

  CartpoleDynamics::state_array x = CartpoleDynamics::state_array::Zero(), x_next = x, xdot = x;
  CartpoleDynamics::output_array y = CartpoleDynamics::output_array::Zero();
  x[0] = 0.3f;
  x[1] = -0.2f;
  x[2] = 0.5f;
  x[3] = 0.1f;

  controller.computeControl(x, 1);
  {
    const auto u_seq = controller.getControlSeq();
    for (int t = 0; t < HORIZON; t++)
      printf("u[%d] = %.9g\n", t, u_seq(0, t));
  }

  for (int i = 0; i < steps; i++)
  {
    if (i > 0)
      controller.computeControl(x, 1);
    CartpoleDynamics::control_array u = controller.getControlSeq().block(0, 0, CartpoleDynamics::CONTROL_DIM, 1);
    model.enforceConstraints(x, u);
    model.step(x, x_next, xdot, u, y, (float)i, dt);
    x = x_next;
    controller.slideControlSequence(1);
  }
  printf("%s with the NLN sampler: %d control steps, pole angle %.4f rad\n", controller.getControllerName().c_str(), steps, x[2]);
  return 0;
}
