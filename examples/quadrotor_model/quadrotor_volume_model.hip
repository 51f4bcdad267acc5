/**
 * quadrotor_volume_model.hip — the registration unit of the quadrotor over a clearance volume: QuadrotorDynamics +
 * QuadrotorVolumeCost (both shipped in include/mppi_amd/), Gaussian sampler, as the model "quadrotor_volume".  The cost is this
 * project's own, not the reference's: QuadrotorQuadraticCost plus a 3-D map read through ThreeDTextureHelper.
 *
 * Compiled on its own into a library and loaded with mppi_load_plugin, exactly as quadrotor_model.hip beside it:
 *   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared -I<repo>/include \
 *         examples/quadrotor_model/quadrotor_volume_model.hip -o libquadrotor_volume_model.so
 * and it stays out of mppi-generic_amd/csrc/models/ for the reason written there.
 *
 * The volume is optional: without the "cost_volume" blob the volume term is 0.  "cost_volume" is {depth, height, width} floats,
 * "cost_volume_transform" origin[3], rotations[9] (row-major), resolution[3] (mppi_set_model_blob).
 *
 * Block shapes and the refused controllers are those of "quadrotor".
 */
#include "mppi_amd/engine/model_registry.hpp"
#include "mppi_amd/sampling_distributions/gaussian.hpp"
#include "mppi_amd/dynamics/quadrotor/quadrotor_dynamics.hpp"
#include "mppi_amd/cost_functions/quadrotor/quadrotor_volume_cost.hpp"

using namespace mppi;
using namespace mppi::engine;

using QuadrotorSampler = sampling_distributions::GaussianDistribution<QuadrotorDynamicsParams>;
using QuadrotorVolumeModel = ModelT<QuadrotorDynamics, QuadrotorVolumeCost, QuadrotorSampler,
                                    Shapes<Shape<64, 1, 1>, Shape<64, 1, 2>, Shape<32, 4, 1>,
                                           /* long horizons (the sample rows of a block live in LDS): */ Shape<16, 1, 1>>,
                                    /*FIN_BY=*/1, void, Shapes<>, /*PIPELINE=*/true>;
MPPI_REGISTER_MODEL("quadrotor_volume", MPPI_SAMPLER_GAUSSIAN, QuadrotorVolumeModel, 64, 1)
