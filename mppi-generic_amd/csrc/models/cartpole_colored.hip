/**
 * cartpole_colored.hip — registered instantiation(s) of libmppi_amd.so: Cartpole + CartpoleQuadraticCost, colored-noise sampler (ColoredMPPI).
 *
 * The analogue of the reference's include/mppi/instantiations/ + src/controllers/ (explicit template instantiations
 * compiled into shared libraries, e.g. src/controllers/cartpole/cartpole_mppi.cu:30-42).  One translation unit per
 * model and sampler, so a new or changed model recompiles alone (buildlib.py compiles the units in parallel).
 *
 * Block shapes (BX rollouts, BY lanes per rollout, BZ systems per launch):
 *   BY == 1 : one lane per rollout, state in VGPRs, no barriers      — analytic models (cartpole, double integrator)
 *   BY  > 1 : the reference's LDS + barrier scheme                     — kept for contract coverage and NN-sized models
 *   BZ == 2 : Tube / RMPPI (actual + nominal system share one launch, tube_mppi_controller.cu:192-209)
 */
#include "mppi_amd/engine/model_registry.hpp"
#include "mppi_amd/sampling_distributions/colored_noise.hpp"
#include "mppi_amd/dynamics/cartpole/cartpole_dynamics.hpp"
#include "mppi_amd/cost_functions/cartpole/cartpole_quadratic_cost.hpp"

using namespace mppi;
using namespace mppi::engine;

/* ColoredMPPI instantiation (reference: controllers/ColoredMPPI/colored_mppi_controller.cuh with
 * ColoredNoiseDistribution as SAMPLING_T): the same plugins with the colored-noise sampler. */
using CartpoleColoredModel =
    ModelT<CartpoleDynamics, CartpoleQuadraticCost, sampling_distributions::ColoredNoiseDistribution<CartpoleDynamicsParams>,
           Shapes<Shape<64, 1, 1>, Shape<64, 4, 1>>, /*FIN_BY=*/1, void, Shapes<>, /*PIPELINE=*/true>;
MPPI_REGISTER_MODEL("cartpole", MPPI_SAMPLER_COLORED, CartpoleColoredModel, 64, 1)

/* Tube with colored noise: one draw per rollout in the rows of both systems, the fused kernel only — a registration of its own,
 * MPPI_CONTROLLER_COLORED's above stays one-system */
using CartpoleColoredTubeModel =
    ModelT<CartpoleDynamics, CartpoleQuadraticCost, sampling_distributions::ColoredNoiseDistribution<CartpoleDynamicsParams>,
           Shapes<Shape<64, 1, 2>>, /*FIN_BY=*/1, void, Shapes<>, /*PIPELINE=*/false>;
MPPI_REGISTER_MODEL("cartpole", MPPI_SAMPLER_COLORED_TUBE, CartpoleColoredTubeModel, 64, 1)
