/**
 * quadrotor_map_model.hip — the registration unit of the gate-racing quadrotor: QuadrotorDynamics + QuadrotorMapCost (both shipped
 * in include/mppi_amd/), Gaussian sampler, as the model "quadrotor_map".
 *
 * Compiled on its own into a library and loaded with mppi_load_plugin, exactly as quadrotor_model.hip beside it:
 *   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared -I<repo>/include \
 *         examples/quadrotor_model/quadrotor_map_model.hip -o libquadrotor_map_model.so
 * and it stays out of mppi-generic_amd/csrc/models/ for the reason written there (the kernel-matrix test files want a builder and
 * a CPU oracle model for every name in the library's own registry, and assume at most two controls).
 *
 * The track map is optional: without the "costmap" blob the map term is 0.  "costmap" is {height, width} floats,
 * "costmap_transform" origin[3], rotations[9] (row-major), resolution[3] (mppi_set_model_blob).
 *
 * Block shapes and the refused controllers are those of "quadrotor".
 */
#include "mppi_amd/engine/model_registry.hpp"
#include "mppi_amd/sampling_distributions/gaussian.hpp"
#include "mppi_amd/dynamics/quadrotor/quadrotor_dynamics.hpp"
#include "mppi_amd/cost_functions/quadrotor/quadrotor_map_cost.hpp"

using namespace mppi;
using namespace mppi::engine;

using QuadrotorSampler = sampling_distributions::GaussianDistribution<QuadrotorDynamicsParams>;
using QuadrotorMapModel = ModelT<QuadrotorDynamics, QuadrotorMapCost, QuadrotorSampler,
                                 Shapes<Shape<64, 1, 1>, Shape<64, 1, 2>, Shape<32, 4, 1>,
                                        /* long horizons (the sample rows of a block live in LDS): */ Shape<16, 1, 1>>,
                                 /*FIN_BY=*/1, void, Shapes<>, /*PIPELINE=*/true>;
MPPI_REGISTER_MODEL("quadrotor_map", MPPI_SAMPLER_GAUSSIAN, QuadrotorMapModel, 64, 1)
