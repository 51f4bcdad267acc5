/**
 * autorally_robust_model.hip — the registration unit of the reference's AutoRally Robust MPPI set-up: NeuralNetModel<7,2,3> +
 * ARRobustCost (both shipped in include/mppi_amd/), Gaussian sampler, as the model "autorally_nn_robust".
 *
 * Compiled on its own into a library and loaded with mppi_load_plugin, exactly as the quadrotor units in examples/quadrotor_model/:
 *   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared -I<repo>/include \
 *         examples/autorally_robust_model/autorally_robust_model.hip -o libautorally_robust_model.so
 * and it stays out of mppi-generic_amd/csrc/models/ for the reason written in quadrotor_map_model.hip (the kernel-matrix test
 * files want a builder and a CPU oracle model for every name in the library's own registry).
 *
 * Blobs (mppi_set_model_blob): "dynamics_weights" as "autorally_nn"; "costmap" is {height, width, 4}
 * interleaved texels — boundary constraint, track position, speed map, heading — and {height, width} is refused.
 * mppi_load_npz(kind "costmap") reads channel0 .. channel3 and interleaves them.  The cost parameter block is
 * mppi_ar_robust_cost_params (model_params.h).
 *
 * Block shapes, the MFMA replicated-lane shapes, FIN_BY and the Robust MPPI instantiation are those of "autorally_nn"
 * (mppi-generic_amd/csrc/models/autorally_nn.hip).
 */
#include "mppi_amd/engine/model_registry.hpp"
#include "mppi_amd/model_params.h"
#include "mppi_amd/sampling_distributions/gaussian.hpp"
#include "mppi_amd/dynamics/autorally/ar_nn_model.hpp"
#include "mppi_amd/cost_functions/autorally/ar_robust_cost.hpp"

using namespace mppi;
using namespace mppi::engine;

static_assert(sizeof(mppi_ar_robust_cost_params) == sizeof(ARRobustCostParams), "POD block and plugin parameters differ");
static_assert(sizeof(mppi_ar_robust_cost_params) == sizeof(mppi_ar_standard_cost_params) + sizeof(float),
              "the robust block is the standard block plus heading_coeff");

using ARModelDyn = NeuralNetModel<7, 2, 3>;
using ARSampler = sampling_distributions::GaussianDistribution<NNDynamicsParams>;
using ARRobustModel = ModelT<ARModelDyn, ARRobustCost, ARSampler,
                             Shapes<Shape<8, 16, 1>, Shape<16, 8, 1>, Shape<16, 4, 1>, Shape<64, 1, 1>, Shape<8, 16, 2>>,
                             /*FIN_BY=*/32,
                             /* MFMA forward: BX rollouts x 4 k-group lanes per block (BX/16 waves) */
                             NeuralNetModelMFMA<7, 2, 3>, Shapes<Shape<64, 4, 1>, Shape<32, 4, 1>, Shape<64, 4, 2>, Shape<32, 4, 2>>,
                             /*PIPELINE=*/false, /*RMPPI=*/true>;
MPPI_REGISTER_MODEL("autorally_nn_robust", MPPI_SAMPLER_GAUSSIAN, ARRobustModel, 64, 4)
