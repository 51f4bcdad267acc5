"""mppi-generic_amd — MI355X-native MPPI rollout-and-reduce engine (host-side Python mirror over the C ABI).

The product is ``lib/libmppi_amd.so`` (hand-written HIP kernels for gfx950 behind include/mppi_amd.h).  This package
only (a) builds it with hipcc, (b) declares its C entry points for ctypes, and (c) mirrors the reference's controller
classes (same method names) on top of those entry points so tests read like the reference's own.
"""
from . import buildlib as _buildlib
from .buildlib import build
from .capi import (MPPI_OK, MPPI_ERR_INVALID_ARG, MPPI_ERR_UNKNOWN_MODEL, MPPI_ERR_NO_DEVICE, MPPI_ERR_HIP, MPPI_ERR_LAUNCH_SHAPE,
                   MPPI_ERR_LDS_OVERFLOW, MPPI_ERR_STATE, MPPI_ERR_NAN, MPPI_ERR_COMM, MPPI_ERR_UNSUPPORTED,
                   MppiTexture2dParams, MppiTexture3dParams, texture3d_query, MppiConfig, MppiGaussianParams, MppiStats, MppiSystemStats, SIGNATURES, library_path, load_library)
from .controllers import (MPPI_KERNEL_AUTO, MPPI_KERNEL_FUSED, MPPI_KERNEL_PIPELINE, MPPI_CONTROLLER_TUBE, MPPI_CONTROLLER_VANILLA, MPPI_NOISE_INJECTED, MPPI_NOISE_PHILOX_FUSED,
                          MPPIError, MPPIController, TubeMPPIController, VanillaMPPIController, ColoredMPPIController, RobustMPPIController,
                          MPPI_CONTROLLER_COLORED, CartpoleDynamicsParams,
                          CartpoleQuadraticCostParams, DoubleIntegratorParams, DoubleIntegratorCircleCostParams,
                          QuadrotorDynamicsParams, QuadrotorQuadraticCostParams, QuadrotorMapCostParams, QuadrotorVolumeCostParams, set_cost_texture, set_cost_volume, det_atan2,
                          ARStandardCostParams, ARRobustCostParams, RacerDubinsParams, RacerDubinsElevationParams, RacerDubinsSuspensionParams, RacerDubinsUncertaintyParams, QuadraticCostParams28, fnn_blob_from_npz_dict, lstm_blob_from_npz_dict,
                          det_eval, LSTMLSTMHelper, texture2d_query, npz_read_array, philox_normal, launch_boundary_us, issue_interval_ns, norm_exp, compute_weights, weighted_reduction,
                          compute_weights_reference_order, weighted_reduction_reference_order,
                          MPPI_REDUCTION_FUSED, MPPI_REDUCTION_REFERENCE_ORDER, MPPI_REDUCTION_REFERENCE_ORDER_FMA,
                          KERNEL_FAMILIES, MPPI_SAMPLER_GAUSSIAN, MPPI_SAMPLER_COLORED, MPPI_SAMPLER_NLN, MPPI_SAMPLER_COLORED_TUBE, list_models, describe_model, sampled_trajectory_list)
from .plant import BasePlant, BufferedPlantMixin, SimulatedPlant, interpolateControls, interpolateFeedback, interpolateState

__all__ = [
    "build", "load_library", "library_path", "MPPIError", "MPPIController", "VanillaMPPIController",
    "TubeMPPIController", "MppiConfig", "SIGNATURES", "BasePlant", "SimulatedPlant",
]
