/**
 * quadrotor_model.hip — the registration unit of the quadrotor: QuadrotorDynamics + QuadrotorQuadraticCost (both shipped in
 * include/mppi_amd/), Gaussian sampler, as the model "quadrotor".
 *
 * Compiled on its own into a library and loaded with mppi_load_plugin, exactly as examples/my_model/pendulum_model.hip:
 *   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared -I<repo>/include \
 *         examples/quadrotor_model/quadrotor_model.hip -o libquadrotor_model.so
 * It is written as a unit of mppi-generic_amd/csrc/models/ and builds into libmppi_amd.so when it is moved there.  It is not there
 * yet because the kernel-matrix test files enumerate the registry of libmppi_amd.so, want a configuration builder and a CPU
 * oracle model for every name in it, and are written for models with one or two controls; this model has four.
 *
 * Block shapes (BX rollouts, BY lanes per rollout, BZ systems per launch):
 *   BY == 1 : one lane per rollout, the 13 states in VGPRs, no barriers
 *   BY == 4 : the reference's shape for this model, dim3(32, 4, 1) (tests/controllers/vanilla_mppi_test.cu:248-249): LDS + barriers
 *   BZ == 2 : Tube MPPI (actual + nominal system share one launch, tube_mppi_controller.cu:192-209)
 *
 * Vanilla and Tube MPPI only: no colored-noise unit (the one-lane colored kernels already spill) and no Robust MPPI
 * (it needs feedback gains nobody has for this model) — mppi_create refuses both.
 */
#include "mppi_amd/engine/model_registry.hpp"
#include "mppi_amd/sampling_distributions/gaussian.hpp"
#include "mppi_amd/dynamics/quadrotor/quadrotor_dynamics.hpp"
#include "mppi_amd/cost_functions/quadrotor/quadrotor_quadratic_cost.hpp"

using namespace mppi;
using namespace mppi::engine;

using QuadrotorSampler = sampling_distributions::GaussianDistribution<QuadrotorDynamicsParams>;
using QuadrotorModel = ModelT<QuadrotorDynamics, QuadrotorQuadraticCost, QuadrotorSampler,
                              Shapes<Shape<64, 1, 1>, Shape<64, 1, 2>, Shape<32, 4, 1>,
                                     /* long horizons (the sample rows of a block live in LDS): */ Shape<16, 1, 1>>,
                              /*FIN_BY=*/1, void, Shapes<>, /*PIPELINE=*/true>;
MPPI_REGISTER_MODEL("quadrotor", MPPI_SAMPLER_GAUSSIAN, QuadrotorModel, 64, 1)
