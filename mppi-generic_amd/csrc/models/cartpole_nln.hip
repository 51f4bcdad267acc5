/**
 * cartpole_nln.hip — registered instantiation(s) of libmppi_amd.so: Cartpole + CartpoleQuadraticCost, NLN sampler (log-MPPI).
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
#include "mppi_amd/sampling_distributions/nln.hpp"
#include "mppi_amd/dynamics/cartpole/cartpole_dynamics.hpp"
#include "mppi_amd/cost_functions/cartpole/cartpole_quadratic_cost.hpp"

using namespace mppi;
using namespace mppi::engine;

/* Any controller of the reference takes NLNDistribution as its SAMPLING_T (sampling_distributions/nln/nln.cuh): the shapes
 * and the role-pipelined kernel of cartpole.hip, streamed merge included, with the NLN draw in the sampler waves. */
using CartpoleNLNModel =
    ModelT<CartpoleDynamics, CartpoleQuadraticCost, sampling_distributions::NLNDistribution<CartpoleDynamicsParams>,
           Shapes<Shape<64, 1, 1>, Shape<64, 1, 2>, Shape<32, 1, 1>, Shape<64, 4, 1>, Shape<16, 4, 1>,
                  /* long horizons (the sample rows of a block live in LDS): */ Shape<16, 1, 1>, Shape<16, 1, 2>>,
           /*FIN_BY=*/1, void, Shapes<>, /*PIPELINE=*/true>;
MPPI_REGISTER_MODEL("cartpole", MPPI_SAMPLER_NLN, CartpoleNLNModel, 64, 1)
