/**
 * double_integrator_nln.hip — registered instantiation(s) of libmppi_amd.so: DoubleIntegrator + DoubleIntegratorCircleCost, NLN sampler (log-MPPI).
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
#include "mppi_amd/dynamics/double_integrator/di_dynamics.hpp"
#include "mppi_amd/cost_functions/double_integrator/double_integrator_circle_cost.hpp"

using namespace mppi;
using namespace mppi::engine;

/* Vanilla and Tube MPPI: the shapes of double_integrator.hip; (32, 1, 2) folded into the lanes of a wave comes with PIPELINE */
using DINLNModel =
    ModelT<DoubleIntegratorDynamics, DoubleIntegratorCircleCost, sampling_distributions::NLNDistribution<DoubleIntegratorParams>,
           Shapes<Shape<64, 1, 1>, Shape<64, 1, 2>, Shape<32, 2, 2>, Shape<64, 2, 1>, Shape<16, 1, 1>, Shape<16, 1, 2>>,
           /*FIN_BY=*/1, void, Shapes<>, /*PIPELINE=*/true>;
MPPI_REGISTER_MODEL("double_integrator", MPPI_SAMPLER_NLN, DINLNModel, 64, 1)
