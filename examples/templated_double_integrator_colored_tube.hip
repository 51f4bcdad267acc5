/**
 * Tube-MPPI with colored noise on the reference's templated host surface: TubeMPPIController with ColoredNoiseDistribution as
 * its SAMPLING_T (the reference: include/mppi/sampling_distributions/colored_noise/colored_noise.cuh handed to the Tube
 * controller template).  One colored draw per rollout serves the actual and the nominal system, the reference's
 * use_same_noise_for_all_distributions.
 *
 * Written against the reference's include paths and class names, like examples/templated_double_integrator.hip: the double
 * integrator on the circle cost, K = 1024, T = 48, dt = 0.02, lambda = 2, noise exponents (1, 0.5).
 *
 * Build:  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I<repo>/include \
 *               examples/templated_double_integrator_colored_tube.hip -L<repo>/mppi-generic_amd/lib -lmppi_amd \
 *               -Wl,-rpath,<repo>/mppi-generic_amd/lib -o templated_double_integrator_colored_tube
 * Run:    ./templated_double_integrator_colored_tube [steps]    `steps` control steps (default 20) with a drifting measured
 *         state, then the sums of the actual and the nominal control sequence ("sum u = ...", "sum u_nominal = ...")
 */
#include <mppi/dynamics/double_integrator/di_dynamics.cuh>
#include <mppi/cost_functions/double_integrator/double_integrator_circle_cost.cuh>
#include <mppi/controllers/Tube-MPPI/tube_mppi_controller.cuh>
#include <mppi/sampling_distributions/colored_noise/colored_noise.cuh>
#include <mppi/feedback_controllers/DDP/ddp.cuh>

#include <cstdio>
#include <cstdlib>

using Dyn = DoubleIntegratorDynamics;
using CircleCost = DoubleIntegratorCircleCost;
constexpr int HORIZON = 48;
constexpr int ROLLOUTS = 1024;
using Feedback = DDPFeedback<Dyn, HORIZON>;
using Sampler = mppi::sampling_distributions::ColoredNoiseDistribution<Dyn::DYN_PARAMS_T>;
using ColoredTube = TubeMPPIController<Dyn, CircleCost, Feedback, HORIZON, ROLLOUTS, Sampler>;

int main(int argc, char** argv)
{
  const int steps = argc > 1 ? atoi(argv[1]) : 20;
  const float dt = 0.02f, lambda = 2.0f, alpha = 0.0f;
  const int max_iter = 1;

  Dyn model;
  CircleCost cost;
  Feedback fb_controller(&model, dt);

  auto sampler_params = Sampler::SAMPLING_PARAMS_T();
  for (int i = 0; i < Dyn::CONTROL_DIM; i++)
    sampler_params.std_dev[i] = 1.0f;
  Sampler sampler;
  sampler.setParams(sampler_params);
  sampler.exponents_[0] = 1.0f;
  sampler.exponents_[1] = 0.5f;

  ColoredTube controller(&model, &cost, &fb_controller, &sampler, dt, max_iter, lambda, alpha);
  controller.setNominalThreshold(20.0f);

  // the measured state drifts by a fixed amount per step (no plant model in between: the printed sums then depend on the
  // controller alone); the nominal system follows its own model and does not see the drift
  Dyn::state_array x = { 2.0f, 0.0f, 0.0f, 1.0f };
  for (int i = 0; i < steps; i++)
  {
    controller.computeControl(x, 1);
    x[0] += 0.01f;
    x[2] += 0.02f;
    if (i + 1 < steps)
      controller.slideControlSequence(1);
  }

  const auto u_seq = controller.getControlSeq();
  const auto un_seq = controller.getNominalControlSeq();
  double sum_u = 0.0, sum_un = 0.0;
  for (int t = 0; t < HORIZON; t++)
    for (int c = 0; c < Dyn::CONTROL_DIM; c++)
    {
      sum_u += (double)u_seq(c, t);
      sum_un += (double)un_seq(c, t);
    }
  printf("%s with colored noise: %d control steps, position (%.6f, %.6f)\n", controller.getControllerName().c_str(), steps, x[0],
         x[1]);
  printf("sum u = %.9g\n", sum_u);
  printf("sum u_nominal = %.9g\n", sum_un);
  return 0;
}
