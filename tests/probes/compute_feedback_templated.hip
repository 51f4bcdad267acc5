/**
 * compute_feedback_templated.hip — TEST CODE: DDPFeedback<CartpoleDynamics, T>::setParams / computeFeedback and the templated
 * controller's computeFeedback(state) (include/mppi_amd/feedback_controllers/ddp_feedback.hpp, controllers_templated.hpp) on the
 * cartpole, written against the reference's include paths.  linearizeKernel and ddpBackwardKernel<4, 1> are instantiated in THIS
 * translation unit, through the ModelT the class registers.  Prints what tests/probes/compute_feedback_host.cpp prints:
 *   points <entries> <sum at two fixed points cycled over the horizon>
 *   trajectory <entries> <sum of computeFeedback(state)'s gains> <sum of mppi_compute_feedback's on the same handle>
 * tests/test_feedback_gpu.py compares the first sum with Python's and the last two with each other.
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

static double checksum(const std::vector<float>& G)
{
  double s = 0.0;
  for (float v : G)
    s += (double)v;
  return s;
}

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

    DDPParams<CartpoleDynamics> fb_params;
    fb_params.Q(0, 0) = 5.0f;
    fb_params.Q(2, 2) = 20.0f;
    fb_params.Q(3, 3) = 2.0f;
    fb_params.R(0, 0) = 0.5f;
    for (int i = 0; i < S; i++)
      fb_params.Q_f(i, i) = 3.0f;
    controller.setFeedbackParams(fb_params);

    const float px[2][S] = { { 0.3f, -0.4f, 0.7f, 1.5f }, { -1.0f, 0.2f, 2.9f, -2.0f } };
    const float pu[2] = { 2.0f, -4.0f };
    CartpoleMPPI::state_trajectory goal = CartpoleMPPI::state_trajectory::Zero();
    CartpoleMPPI::control_trajectory ctrl = CartpoleMPPI::control_trajectory::Zero();
    for (int t = 0; t < HORIZON; t++)
    {
      for (int i = 0; i < S; i++)
        goal(i, t) = px[t % 2][i];
      ctrl(0, t) = pu[t % 2];
    }
    CartpoleMPPI::state_array x0 = CartpoleMPPI::state_array::Zero();
    x0[2] = 0.5f;
    (void)controller.handle();  // the controller creates its engine handle and binds it to the feedback object
    fb_controller.computeFeedback(x0, goal, ctrl);
    printf("points %zu %.17g\n", fb_controller.getFeedbackGains().size(), checksum(fb_controller.getFeedbackGains()));

    controller.computeControl(x0, 1);
    controller.computeFeedback(x0);
    std::vector<float> G((size_t)HORIZON * S * C);
    if (mppi_compute_feedback(controller.handle(), 0, G.data()) != MPPI_OK)
      throw std::runtime_error(mppi_last_error(controller.handle()));
    printf("trajectory %zu %.17g %.17g\n", fb_controller.getFeedbackGains().size(), checksum(fb_controller.getFeedbackGains()),
           checksum(G));
    return 0;
  }
  catch (const std::exception& e)
  {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}
