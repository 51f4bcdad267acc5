"""Host-side mirror of the reference's controller classes over the C ABI.

Method names follow the reference (controllers/controller.cuh, controllers/MPPI/mppi_controller.cuh,
controllers/Tube-MPPI/tube_mppi_controller.cuh): computeControl, getControlSeq, getTargetStateSeq,
slideControlSequence, updateImportanceSampler, getBaselineCost, getNormalizerCost, ...
All numerics happen in libmppi_amd.so; arrays are numpy float32, row-major ([T][C], [T][S], [K][T][C]).
"""
import ctypes as C

import numpy as np

from .capi import (MPPI_ERR_INVALID_ARG, MPPI_ERR_UNKNOWN_MODEL, MppiConfig, MppiGaussianParams, MppiLaunchInfo, MppiStats,
                   load_library)

MPPI_CONTROLLER_VANILLA = 0
MPPI_CONTROLLER_TUBE = 1
MPPI_CONTROLLER_ROBUST = 2
MPPI_CONTROLLER_COLORED = 3
MPPI_NOISE_PHILOX_FUSED = 0
MPPI_NOISE_INJECTED = 1
MPPI_NOISE_ROCRAND_HOST = 2
MPPI_KERNEL_AUTO, MPPI_KERNEL_FUSED, MPPI_KERNEL_PIPELINE = 0, 1, 2
MPPI_REDUCTION_FUSED, MPPI_REDUCTION_REFERENCE_ORDER, MPPI_REDUCTION_REFERENCE_ORDER_FMA = 0, 1, 2


class MPPIError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("mppi status %d: %s" % (status, message))
        self.status = status


# ---- POD parameter blocks (include/mppi_amd/model_params.h) -------------------------------------------------------
class CartpoleDynamicsParams(C.Structure):
    _fields_ = [("cart_mass", C.c_float), ("pole_mass", C.c_float), ("pole_length", C.c_float)]

    def __init__(self, cart_mass=1.0, pole_mass=1.0, pole_length=1.0):
        super().__init__(cart_mass, pole_mass, pole_length)


class CartpoleQuadraticCostParams(C.Structure):
    _fields_ = [
        ("control_cost_coeff", C.c_float * 1), ("discount", C.c_float),
        ("cart_position_coeff", C.c_float), ("cart_velocity_coeff", C.c_float), ("pole_angle_coeff", C.c_float),
        ("pole_angular_velocity_coeff", C.c_float), ("terminal_cost_coeff", C.c_float),
        ("desired_terminal_state", C.c_float * 4),
    ]

    def __init__(self):
        super().__init__()
        self.control_cost_coeff[0] = 10.0
        self.discount = 1.0
        self.cart_position_coeff = 1000
        self.cart_velocity_coeff = 100
        self.pole_angle_coeff = 2000
        self.pole_angular_velocity_coeff = 100
        self.terminal_cost_coeff = 0
        self.desired_terminal_state[:] = [0.0, 0.0, np.float32(np.pi), 0.0]


class DoubleIntegratorParams(C.Structure):
    _fields_ = [("system_noise", C.c_float)]

    def __init__(self, system_noise=1.0):
        super().__init__(system_noise)


class DoubleIntegratorCircleCostParams(C.Structure):
    _fields_ = [
        ("control_cost_coeff", C.c_float * 2), ("discount", C.c_float), ("velocity_cost", C.c_float),
        ("crash_cost", C.c_float), ("velocity_desired", C.c_float), ("inner_path_radius2", C.c_float),
        ("outer_path_radius2", C.c_float), ("angular_momentum_desired", C.c_float),
    ]

    def __init__(self):
        super().__init__()
        self.control_cost_coeff[:] = [0.01, 0.01]
        self.discount = 1.0
        self.velocity_cost = 1
        self.crash_cost = 1000
        self.velocity_desired = 2
        self.inner_path_radius2 = 1.875 * 1.875
        self.outer_path_radius2 = 2.125 * 2.125
        self.angular_momentum_desired = 4


class QuadrotorDynamicsParams(C.Structure):
    """mppi_quadrotor_dynamics_params (reference: dynamics/quadrotor/quadrotor_dynamics.cuh:10-63)"""
    _fields_ = [("tau_roll", C.c_float), ("tau_pitch", C.c_float), ("tau_yaw", C.c_float), ("mass", C.c_float)]

    def __init__(self, mass=1.0):
        super().__init__(0.25, 0.25, 0.25, mass)


class QuadrotorQuadraticCostParams(C.Structure):
    """mppi_quadrotor_cost_params (reference: cost_functions/quadrotor/quadrotor_quadratic_cost.cuh:10-70); s_goal is
    position, velocity, quaternion (w x y z), body rates"""
    _fields_ = [
        ("control_cost_coeff", C.c_float * 4), ("discount", C.c_float), ("s_goal", C.c_float * 13),
        ("x_coeff", C.c_float), ("v_coeff", C.c_float), ("use_euler", C.c_int), ("q_coeff", C.c_float),
        ("roll_coeff", C.c_float), ("pitch_coeff", C.c_float), ("yaw_coeff", C.c_float), ("w_coeff", C.c_float),
        ("terminal_cost_coeff", C.c_float),
    ]

    def __init__(self):
        super().__init__()
        self.control_cost_coeff[:] = [2.0] * 4
        self.discount = 1.0
        self.s_goal[:] = [0.0] * 6 + [1.0] + [0.0] * 6
        self.x_coeff = self.v_coeff = self.q_coeff = self.w_coeff = 1.0
        self.roll_coeff = self.pitch_coeff = self.yaw_coeff = 1.0
        self.use_euler = 1
        self.terminal_cost_coeff = 0.0


def _libm_f32(name):
    """cosf / sinf of the C library, which the reference's host code and the C++ updateWaypoint call.  Looked up at the first
    call; without a C math library it raises — another float32 cosine may differ in the last bit, and the gate posts would then
    quietly stop matching the C++ class's"""
    fn = []

    def call(a):
        if not fn:
            import ctypes.util
            try:
                f = getattr(C.CDLL(ctypes.util.find_library("m") or "libm.so.6"), name)
            except (OSError, AttributeError) as e:
                raise OSError("QuadrotorMapCostParams.update_waypoint needs %s of the C math library: %s" % (name, e)) from e
            f.restype, f.argtypes = C.c_float, [C.c_float]
            fn.append(f)
        return np.float32(fn[0](float(a)))
    return call


_cosf, _sinf = _libm_f32("cosf"), _libm_f32("sinf")


class QuadrotorMapCostParams(C.Structure):
    """mppi_quadrotor_map_cost_params (reference: cost_functions/quadrotor/quadrotor_map_cost.cuh:14-91); waypoints are
    x, y, z, heading.  r_c1 / r_c2 / trs belong to the reference's legacy texture path and are unused; the track map and its frame
    are the "costmap" / "costmap_transform" blobs (set_cost_texture)."""
    _fields_ = [
        ("control_cost_coeff", C.c_float * 4), ("discount", C.c_float),
        ("r_c1", C.c_float * 3), ("r_c2", C.c_float * 3), ("trs", C.c_float * 3),
        ("attitude_coeff", C.c_float), ("crash_coeff", C.c_float), ("dist_to_waypoint_coeff", C.c_float),
        ("heading_coeff", C.c_float), ("heading_power", C.c_float), ("height_coeff", C.c_float), ("track_coeff", C.c_float),
        ("speed_coeff", C.c_float), ("track_slop", C.c_float), ("gate_pass_cost", C.c_float),
        ("curr_waypoint", C.c_float * 4), ("prev_waypoint", C.c_float * 4), ("curr_gate_left", C.c_float * 3),
        ("curr_gate_right", C.c_float * 3), ("prev_gate_left", C.c_float * 3), ("prev_gate_right", C.c_float * 3),
        ("end_waypoint", C.c_float * 4),
        ("desired_speed", C.c_float), ("gate_margin", C.c_float), ("min_dist_to_gate_side", C.c_float),
        ("track_boundary_cost", C.c_float), ("gate_width", C.c_float),
    ]

    def __init__(self):
        super().__init__()
        self.control_cost_coeff[:] = [1.0] * 4
        self.discount = 1.0
        self.r_c1[:], self.r_c2[:], self.trs[:] = [1, 0, 0], [0, 1, 0], [0, 0, 1]
        self.attitude_coeff, self.crash_coeff, self.dist_to_waypoint_coeff = 10, 1000, 0.0
        self.heading_coeff, self.heading_power, self.height_coeff = 5, 1.0, 5
        self.track_coeff, self.speed_coeff, self.track_slop, self.gate_pass_cost = 10, 5, 0.0, -150
        self.end_waypoint[:] = [float("nan")] * 4
        self.desired_speed, self.gate_margin, self.min_dist_to_gate_side = 5, 0.5, 0.5
        self.track_boundary_cost, self.gate_width = 2.5, 2.15

    def update_waypoint(self, x, y, z, heading=0.0):
        """QuadrotorMapCostParams::updateWaypoint (quadrotor_map_cost.cuh:62-75): a new waypoint moves current to previous and
        places the gate's posts gate_width to either side along the heading, in float32 with the C library's cosf / sinf;
        the same waypoint again changes nothing.  Returns whether it changed — push the block with setCostParams then."""
        new = [np.float32(v) for v in (x, y, z, heading)]
        if not any(np.float32(a) != b for a, b in zip(self.curr_waypoint, new)):
            return False
        self.prev_waypoint[:] = list(self.curr_waypoint)
        self.curr_waypoint[:] = new
        x, y, z, heading = new
        gw, c, s = np.float32(self.gate_width), _cosf(heading), _sinf(heading)
        self.update_gate_boundaries(x + c * gw, y + s * gw, z, x - c * gw, y - s * gw, z)
        return True

    def update_gate_boundaries(self, left_x, left_y, left_z, right_x, right_y, right_z):
        """QuadrotorMapCostParams::updateGateBoundaries (quadrotor_map_cost.cuh:77-90)"""
        left = [np.float32(v) for v in (left_x, left_y, left_z)]
        right = [np.float32(v) for v in (right_x, right_y, right_z)]
        if not any(np.float32(a) != b for a, b in zip(list(self.curr_gate_left) + list(self.curr_gate_right), left + right)):
            return False
        self.prev_gate_left[:] = list(self.curr_gate_left)
        self.prev_gate_right[:] = list(self.curr_gate_right)
        self.curr_gate_left[:] = left
        self.curr_gate_right[:] = right
        return True


def set_cost_texture(controller, costmap, origin=(0.0, 0.0, 0.0), rotations=None, resolution=(1.0, 1.0, 1.0)):
    """the map of a cost that samples it through a TwoDTextureHelper (QuadrotorMapCost): costmap [height][width], and its frame
    — world origin of the map, world -> map rotation (3 x 3, row-major; identity when None), metres per texel — as the
    "costmap" and "costmap_transform" blobs of mppi_set_model_blob"""
    cm = _f32(costmap)
    assert cm.ndim == 2, cm.shape
    rot = np.eye(3, dtype=np.float32) if rotations is None else _f32(rotations).reshape(3, 3)
    frame = np.concatenate([_f32(origin).reshape(3), rot.reshape(9), _f32(resolution).reshape(3)])
    controller.setModelBlob("costmap_transform", frame)
    controller.setModelBlob("costmap", cm)


class QuadrotorVolumeCostParams(C.Structure):
    """mppi_quadrotor_volume_cost_params (QuadrotorVolumeCost, not in the reference): QuadrotorQuadraticCostParams and the three
    fields of the clearance-volume term, volume_coeff * max(0, v) and crash_coeff where v > crash_threshold; the volume and its
    frame are the "cost_volume" / "cost_volume_transform" blobs (set_cost_volume)."""
    _fields_ = QuadrotorQuadraticCostParams._fields_ + [("volume_coeff", C.c_float), ("crash_threshold", C.c_float),
                                                        ("crash_coeff", C.c_float)]

    def __init__(self):
        super().__init__()
        self.control_cost_coeff[:] = [2.0] * 4
        self.discount = 1.0
        self.s_goal[:] = [0.0] * 6 + [1.0] + [0.0] * 6
        self.x_coeff = self.v_coeff = self.q_coeff = self.w_coeff = 1.0
        self.roll_coeff = self.pitch_coeff = self.yaw_coeff = 1.0
        self.use_euler = 1
        self.terminal_cost_coeff = 0.0
        self.volume_coeff, self.crash_threshold, self.crash_coeff = 10.0, 0.9, 1000.0


def set_cost_volume(controller, volume, origin=(0.0, 0.0, 0.0), rotations=None, resolution=(1.0, 1.0, 1.0)):
    """the volume of a cost that samples it through a ThreeDTextureHelper (QuadrotorVolumeCost): volume [depth][height][width],
    and its frame as in set_cost_texture, as the "cost_volume" and "cost_volume_transform" blobs of mppi_set_model_blob"""
    v = _f32(volume)
    assert v.ndim == 3, v.shape
    rot = np.eye(3, dtype=np.float32) if rotations is None else _f32(rotations).reshape(3, 3)
    frame = np.concatenate([_f32(origin).reshape(3), rot.reshape(9), _f32(resolution).reshape(3)])
    controller.setModelBlob("cost_volume_transform", frame)
    controller.setModelBlob("cost_volume", v)


class RacerDubinsParams(C.Structure):
    """mppi_racer_dubins_params (reference: dynamics/racer_dubins/racer_dubins.cuh:67-87)"""
    _fields_ = [("c_t", C.c_float * 3), ("c_b", C.c_float * 3), ("c_v", C.c_float * 3), ("c_0", C.c_float),
                ("steering_constant", C.c_float), ("steer_command_angle_scale", C.c_float), ("steer_angle_scale", C.c_float),
                ("max_steer_angle", C.c_float), ("max_steer_rate", C.c_float), ("steer_accel_constant", C.c_float),
                ("steer_accel_drag_constant", C.c_float), ("brake_delay_constant", C.c_float),
                ("brake_delay_constant_neg", C.c_float), ("max_brake_rate_neg", C.c_float), ("max_brake_rate_pos", C.c_float),
                ("wheel_base", C.c_float), ("low_min_throttle", C.c_float), ("gravity", C.c_float), ("gear_sign", C.c_int)]

    def __init__(self):
        super().__init__()
        self.c_t[:] = [1.3, 2.6, 3.9]
        self.c_b[:] = [2.5, 3.5, 4.5]
        self.c_v[:] = [3.7, 4.7, 5.7]
        self.c_0 = 4.9
        self.steering_constant = 0.6
        self.steer_command_angle_scale = 5
        self.steer_angle_scale = -9.1
        self.max_steer_angle = 0.5
        self.max_steer_rate = 5
        self.steer_accel_constant = 12.1
        self.steer_accel_drag_constant = 1.0
        self.brake_delay_constant = 6.6
        self.brake_delay_constant_neg = 8.2
        self.max_brake_rate_neg = 0.9
        self.max_brake_rate_pos = 0.33
        self.wheel_base = 0.3
        self.low_min_throttle = 0.13
        self.gravity = -9.81
        self.gear_sign = 1


class RacerDubinsElevationParams(C.Structure):
    """mppi_racer_dubins_elevation_params (reference: dynamics/racer_dubins/racer_dubins_elevation.cuh:16-60)"""
    _fields_ = [("base", RacerDubinsParams), ("clamp_ax", C.c_float), ("K_x", C.c_float), ("K_y", C.c_float),
                ("K_yaw", C.c_float), ("K_vel_x", C.c_float), ("Q_x_acc", C.c_float), ("Q_x_v", C.c_float * 3),
                ("Q_y_f", C.c_float), ("Q_omega_v", C.c_float), ("Q_omega_steering", C.c_float)]

    def __init__(self):
        super().__init__()
        RacerDubinsParams.__init__(self.base)
        self.clamp_ax = 5.5
        self.K_x = self.K_y = self.K_yaw = self.K_vel_x = 1.0
        self.Q_x_acc = 1.0
        self.Q_x_v[:] = [41.74219, -0.8187027, -2.2131343]
        self.Q_y_f = 0.1
        self.Q_omega_v = 0.001
        self.Q_omega_steering = 0.0


class RacerDubinsSuspensionParams(C.Structure):
    """mppi_racer_dubins_suspension_params (reference: dynamics/racer_dubins/racer_dubins_elevation_suspension_lstm.cuh:17-66)"""
    _fields_ = [("elevation", RacerDubinsElevationParams), ("spring_k", C.c_float), ("drag_c", C.c_float),
                ("mass", C.c_float), ("I_xx", C.c_float), ("I_yy", C.c_float), ("wheel_radius", C.c_float),
                ("c_g", C.c_float * 3)]

    def __init__(self):
        super().__init__()
        RacerDubinsElevationParams.__init__(self.elevation)
        self.spring_k, self.drag_c, self.mass = 14000.0, 1000.0, 1447.0
        self.I_xx = np.float32(1.0) / np.float32(12) * np.float32(1447.0) * np.float32(2) * np.float32(2.25)
        self.I_yy = np.float32(1.0) / np.float32(12) * np.float32(1447.0) * np.float32(11.25)
        self.wheel_radius = 0.32
        self.c_g[:] = [2.981 * 0.5, 0.0, 0.0]

    @property
    def base(self):
        return self.elevation.base


class RacerDubinsUncertaintyParams(C.Structure):
    """mppi_racer_dubins_uncertainty_params (reference: dynamics/racer_dubins/racer_dubins_elevation_lstm_unc.cuh:5-48)"""
    _fields_ = [("suspension", RacerDubinsSuspensionParams), ("unc_scale", C.c_float * 7),
                ("pos_quad_brake_c", C.c_float * 3), ("neg_quad_brake_c", C.c_float * 3), ("use_static_settling", C.c_int)]

    def __init__(self):
        super().__init__()
        RacerDubinsSuspensionParams.__init__(self.suspension)
        self.unc_scale[:] = [1.0] * 7
        self.pos_quad_brake_c[:] = [2.0, 0.5, 0.3]
        self.neg_quad_brake_c[:] = [5.84, 0.15, 1.7]
        self.use_static_settling = 1

    @property
    def base(self):
        return self.suspension.elevation.base

    @property
    def elevation(self):
        return self.suspension.elevation


class QuadraticCostParams28(C.Structure):
    """mppi_quadratic_cost_params_28 (reference: QuadraticCostTrajectoryParams<RacerDubins, 1>,
    cost_functions/quadratic_cost/quadratic_cost.cuh:11-63)"""
    _fields_ = [("control_cost_coeff", C.c_float * 2), ("discount", C.c_float), ("s_goal", C.c_float * 28),
                ("s_coeffs", C.c_float * 28), ("current_time", C.c_int)]

    def __init__(self):
        super().__init__()
        self.discount = 1.0
        self.s_coeffs[:] = [1.0] * 28


class ARStandardCostParams(C.Structure):
    _fields_ = [
        ("control_cost_coeff", C.c_float * 2), ("discount", C.c_float), ("desired_speed", C.c_float),
        ("speed_coeff", C.c_float), ("track_coeff", C.c_float), ("max_slip_ang", C.c_float),
        ("slip_coeff", C.c_float), ("track_slop", C.c_float), ("crash_coeff", C.c_float),
        ("boundary_threshold", C.c_float), ("grid_res", C.c_int), ("r_c1", C.c_float * 3), ("r_c2", C.c_float * 3),
        ("trs", C.c_float * 3),
    ]

    def __init__(self):
        super().__init__()
        self.control_cost_coeff[:] = [0.0, 0.0]
        self.discount = 1.0
        self.desired_speed = 6.0
        self.speed_coeff = 4.25
        self.track_coeff = 200.0
        self.max_slip_ang = 1.25
        self.slip_coeff = 10.0
        self.track_slop = 0
        self.crash_coeff = 10000
        self.boundary_threshold = 0.65
        self.grid_res = 10
        self.r_c1[:] = [1, 0, 0]
        self.r_c2[:] = [0, 1, 0]
        self.trs[:] = [0, 0, 1]

    def setTransformFromBounds(self, x_min, x_max, y_min, y_max):
        """the transform ARStandardCost::loadTrackData builds (ar_standard_cost.cu:132-137)"""
        self.r_c1[:] = [1.0 / (x_max - x_min), 0, 0]
        self.r_c2[:] = [0, 1.0 / (y_max - y_min), 0]
        self.trs[:] = [-x_min / (x_max - x_min), -y_min / (y_max - y_min), 1]


class ARRobustCostParams(C.Structure):
    """mppi_ar_robust_cost_params (reference: cost_functions/autorally/ar_robust_cost.cuh:6-29): ARStandardCostParams' fields with
    the robust cost's defaults, then heading_coeff.  The model's "costmap" blob is [height][width][4] interleaved texels
    (boundary constraint, track position, speed map, heading)."""
    _fields_ = ARStandardCostParams._fields_ + [("heading_coeff", C.c_float)]

    def __init__(self):
        super().__init__()
        self.control_cost_coeff[:] = [0.0, 0.0]
        self.discount = 1.0
        self.desired_speed = -1
        self.speed_coeff = 20.0
        self.track_coeff = 33.0
        self.max_slip_ang = 1.5
        self.slip_coeff = 0.0
        self.track_slop = 0
        self.crash_coeff = 125000
        self.boundary_threshold = 0.75
        self.grid_res = 10
        self.r_c1[:] = [1, 0, 0]
        self.r_c2[:] = [0, 1, 0]
        self.trs[:] = [0, 0, 1]
        self.heading_coeff = 0.0

    setTransformFromBounds = ARStandardCostParams.setTransformFromBounds


def fnn_blob_from_npz_dict(d, prefix="dynamics_"):
    """flat FNN parameter blob [W1|b1|W2|b2|...] from the reference's .npz key layout (dynamics_W{i}, dynamics_b{i},
    float64; FNNHelper::loadParams, utils/nn_helpers/fnn_helper.cu:96-174)"""
    parts, i = [], 1
    while prefix + "W%d" % i in d:
        parts.append(np.asarray(d[prefix + "W%d" % i], np.float64).reshape(-1))
        parts.append(np.asarray(d[prefix + "b%d" % i], np.float64).reshape(-1))
        i += 1
    return np.concatenate(parts).astype(np.float32)


def lstm_blob_from_npz_dict(d, prefix=""):
    """LSTM parameter blob [W_im W_fm W_om W_cm | W_ii W_fi W_oi W_ci | b_i b_f b_o b_c | h0 | c0] from the reference's
    .npz key layout ({prefix}lstm/weight_hh_l0, weight_ih_l0, bias_hh_l0, bias_ih_l0, float64, PyTorch gate order
    i, f, g, o; LSTMHelper::loadParams, utils/nn_helpers/lstm_helper.cu:514-578: gates re-ordered to i, f, o, c and the
    two bias vectors summed).  Optional keys {prefix}lstm/h0, c0 give the initial state (default zeros).
    Returns (lstm_blob, output_fnn_blob); the output network uses the keys {prefix}output/dynamics_W{i}, _b{i}."""
    if prefix and not prefix.endswith("/"):
        prefix += "/"
    if "model/" + prefix + "lstm/weight_hh_l0" in d:
        prefix = "model/" + prefix
    whh = np.asarray(d[prefix + "lstm/weight_hh_l0"], np.float64)
    wih = np.asarray(d[prefix + "lstm/weight_ih_l0"], np.float64)
    b = np.asarray(d[prefix + "lstm/bias_hh_l0"], np.float64) + np.asarray(d[prefix + "lstm/bias_ih_l0"], np.float64)
    H = b.size // 4
    order = [0, 1, 3, 2]  # blob gate g <- torch gate order[g]  (i, f, o, c  <-  i, f, g(c), o)
    parts = [whh[g * H:(g + 1) * H].reshape(-1) for g in order]
    parts += [wih[g * H:(g + 1) * H].reshape(-1) for g in order]
    parts += [b[g * H:(g + 1) * H] for g in order]
    parts.append(np.asarray(d.get(prefix + "lstm/h0", np.zeros(H)), np.float64).reshape(-1))
    parts.append(np.asarray(d.get(prefix + "lstm/c0", np.zeros(H)), np.float64).reshape(-1))
    return np.concatenate(parts).astype(np.float32), fnn_blob_from_npz_dict(d, prefix + "output/dynamics_")


def sampled_trajectory_list(num_rollouts, fraction=0.0, seed=None):
    """the random part of the reference's sampled-trajectory list (controllers/controller.cu:63-84) as local rollout indices:
    -1 (slot 0, the optimal sequence), then int(fraction * K) indices drawn without replacement from the first 98 % of the
    rollouts — 0, 1, 2, ... when fraction > 0.98, as there — with numpy's default generator seeded with `seed`"""
    k = int(num_rollouts)
    m = min(int(fraction * k), k) if fraction > 0 else 0
    if m <= 0:
        drawn = np.empty(0, np.int32)
    elif fraction > 0.98:
        drawn = np.arange(m, dtype=np.int32)
    else:
        pool = int(k * 0.98)
        drawn = np.random.default_rng(seed).choice(pool, size=min(m, pool), replace=False).astype(np.int32)
    return np.concatenate([np.array([-1], np.int32), drawn])


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


class MPPIController:
    """Common part of the reference's Controller<DYN, COST, FB, SAMPLING, MAX_TIMESTEPS, NUM_ROLLOUTS>.

    A controller object is not thread-safe: computeControl, getControlSeq and slideControlSequence share staging arrays,
    and the handle underneath holds one control sequence.  Calls on one object come from one thread at a time."""

    KIND = MPPI_CONTROLLER_VANILLA

    def __init__(self, model, num_rollouts, num_timesteps, dt, lambda_, alpha=0.0, num_iters=1, seed=42,
                 noise_source=MPPI_NOISE_PHILOX_FUSED, block_x=0, block_y=0, device=0, stream=None, rank=0,
                 world_size=1, save_samples=False, kernel_variant=0, force_exchange=False, sampler=None):
        """sampler: an MPPI_SAMPLER_* constant, the reference's SAMPLING_T.  None is the controller's own (Gaussian; colored noise
        for ColoredMPPIController); the Vanilla, Tube and Robust controllers also take MPPI_SAMPLER_NLN (log-MPPI), and
        TubeMPPIController takes MPPI_SAMPLER_COLORED (one colored draw per rollout, shared by both systems)."""
        self._lib = load_library()
        self._h = C.c_void_p()
        self._model = model.encode()
        cfg = MppiConfig(self._model, self.KIND, num_rollouts, num_timesteps, dt, lambda_, alpha, num_iters, seed,
                         noise_source, block_x, block_y, device, stream, rank, world_size, int(save_samples), kernel_variant,
                         int(force_exchange))
        if sampler is None:
            st = self._lib.mppi_create(C.byref(cfg), C.byref(self._h))
        else:
            st = self._lib.mppi_create_with_sampler(C.byref(cfg), int(sampler), C.byref(self._h))
        if st != 0:
            self._h = C.c_void_p()
            raise MPPIError(st, (self._lib.mppi_last_error(None) or b"").decode())
        s, c, o, d = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self._check(self._lib.mppi_get_dims(self._h, C.byref(s), C.byref(c), C.byref(o), C.byref(d)))
        self.STATE_DIM, self.CONTROL_DIM, self.OUTPUT_DIM, self.num_systems = s.value, c.value, o.value, d.value
        kl, ko = C.c_int(), C.c_int()
        self._check(self._lib.mppi_get_local_rollouts(self._h, C.byref(kl), C.byref(ko)))
        self.num_rollouts_local, self.rollout_offset = kl.value, ko.value
        self.num_rollouts, self.num_timesteps = num_rollouts, num_timesteps
        self.dt, self.lambda_, self.alpha = dt, lambda_, alpha
        self.sampler = self._lib.mppi_get_sampler_kind(self._h)
        self._init_fast_calls()

    def _init_fast_calls(self):
        """The three calls a control loop makes every cycle (computeControl, getControlSeq, slide) with raw-pointer signatures and
        persistent staging arrays: a numpy.ctypeslib.ndpointer argument costs ~3.3 us of marshalling PER CALL on this class of
        host (measured: 3.31 us against 0.21 us for an integer address) — 7-8 us of a 45 us closed-loop cycle were this wrapper,
        not the engine.  Same library entry points, same values; everything else keeps the checked ndpointer signatures."""
        def raw(name, *argtypes):
            addr = C.cast(getattr(self._lib, name), C.c_void_p).value
            return C.CFUNCTYPE(C.c_int, *argtypes)(addr)
        self._fast_compute = raw("mppi_compute_control", C.c_void_p, C.c_void_p, C.c_int)
        self._fast_get_control = raw("mppi_get_control_seq", C.c_void_p, C.c_void_p)
        self._fast_slide = raw("mppi_slide", C.c_void_p, C.c_int)
        self._hv = self._h.value
        self._x_stage = np.zeros(self.STATE_DIM, np.float32)
        self._x_ptr = self._x_stage.ctypes.data
        self._u_stage = np.empty((self.num_timesteps, self.CONTROL_DIM), np.float32)
        self._u_ptr = self._u_stage.ctypes.data

    def launchCounts(self):
        """(rollout launches, reduction-stage launches) of this handle since creation (mppi_get_launch_counts)"""
        r, g = C.c_ulonglong(), C.c_ulonglong()
        self._check(self._lib.mppi_get_launch_counts(self._h, C.byref(r), C.byref(g)))
        return r.value, g.value

    def getLaunchInfo(self):
        """the most recent rollout launch as the launch path recorded it (mppi_get_launch_info): dict with "family" (a
        KERNEL_FAMILIES name), "block" (bx, by, bz), "rows_in_hbm" and "streamed_merge"; MPPIError(MPPI_ERR_STATE) before the
        first launch"""
        info = MppiLaunchInfo()
        self._check(self._lib.mppi_get_launch_info(self._h, C.byref(info)))
        return {"family": KERNEL_FAMILIES[info.family], "block": (info.block_x, info.block_y, info.block_z),
                "rows_in_hbm": bool(info.rows_in_hbm), "streamed_merge": bool(info.streamed_merge)}

    # -- plumbing --
    def _check(self, st):
        if st != 0:
            raise MPPIError(st, (self._lib.mppi_last_error(self._h) or b"").decode())

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.mppi_destroy(self._h)
            self._h = C.c_void_p()
            self._hv = None  # (a call on a closed controller reaches the library with a null handle: MPPI_ERR_INVALID_ARG)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- parameters --
    def setDynamicsParams(self, pod):
        self._check(self._lib.mppi_set_dynamics_params(self._h, C.byref(pod), C.sizeof(pod)))

    def setCostParams(self, pod):
        self._check(self._lib.mppi_set_cost_params(self._h, C.byref(pod), C.sizeof(pod)))

    def setSamplingParams(self, std_dev, control_cost_coeff=None, pure_noise_trajectories_percentage=0.01,
                          std_dev_decay=1.0, sum_strides=32):
        sd = _f32(std_dev).reshape(-1)
        if sd.size == self.CONTROL_DIM and self.num_systems == 2:
            sd = np.concatenate([sd, sd])
        cc = _f32(np.zeros(self.CONTROL_DIM) if control_cost_coeff is None else control_cost_coeff).reshape(-1)
        p = MppiGaussianParams(sd.ctypes.data_as(C.POINTER(C.c_float)), cc.ctypes.data_as(C.POINTER(C.c_float)),
                               pure_noise_trajectories_percentage, std_dev_decay, sum_strides)
        self._check(self._lib.mppi_set_sampler_params(self._h, C.byref(p)))

    def setTimeSpecificStdDev(self, std_dev):
        """std_dev [D][T][C] (or [T][C] for one distribution), None switches back to one sigma per control"""
        if std_dev is None:
            self._check(self._lib.mppi_set_time_specific_std_dev(self._h, None))
            return
        a = _f32(std_dev).reshape(-1)
        assert a.size == self.num_systems * self.num_timesteps * self.CONTROL_DIM, a.size
        self._check(self._lib.mppi_set_time_specific_std_dev(self._h, a.ctypes.data))

    def setModelBlob(self, name, array):
        """bulk model data (NN weights, costmap) — see mppi_set_model_blob"""
        a = _f32(array)
        dims = (C.c_int * a.ndim)(*a.shape)
        self._check(self._lib.mppi_set_model_blob(self._h, name.encode(), a.reshape(-1), a.size, dims, a.ndim))

    def setLSTMInitialState(self, hidden, cell):
        """new initial hidden / cell state of the rollouts' LSTM (LSTMHelper::setHiddenState / setCellState +
        copyHiddenCellToDevice, utils/nn_helpers/lstm_helper.cu:476-500)"""
        self._check(self._lib.mppi_set_lstm_initial_state(self._h, _f32(hidden).reshape(-1), _f32(cell).reshape(-1)))

    def loadNpz(self, kind, path, prefix=None):
        """model data straight from the reference's .npz layout (kind: "dynamics" | "lstm" | "costmap"); mppi_load_npz"""
        self._check(self._lib.mppi_load_npz(self._h, kind.encode(), str(path).encode(),
                                            None if prefix is None else prefix.encode()))

    def setControlRanges(self, lo_hi):
        self._check(self._lib.mppi_set_control_ranges(self._h, _f32(lo_hi).reshape(-1)))

    def setControlDeadbands(self, db):
        self._check(self._lib.mppi_set_control_deadband(self._h, _f32(db).reshape(-1)))

    def setLambda(self, lambda_):
        self.lambda_ = lambda_
        self._check(self._lib.mppi_set_lambda_alpha(self._h, self.lambda_, self.alpha))

    def setNumIters(self, n):
        self._check(self._lib.mppi_set_num_iters(self._h, n))

    def setReductionMode(self, mode):
        """MPPI_REDUCTION_FUSED (default) | MPPI_REDUCTION_REFERENCE_ORDER | MPPI_REDUCTION_REFERENCE_ORDER_FMA:
        mppi_set_reduction_mode — the last stage of an iteration in the reference's own arithmetic order"""
        self._check(self._lib.mppi_set_reduction_mode(self._h, int(mode)))

    def setSlideControlScale(self, scale):
        self._check(self._lib.mppi_set_slide_control_scale(self._h, _f32(scale).reshape(-1)))

    def setSeed(self, seed):
        self._check(self._lib.mppi_set_seed(self._h, seed))

    # -- control loop --
    def updateImportanceSampler(self, u):
        u = _f32(u)
        assert u.shape == (self.num_timesteps, self.CONTROL_DIM)
        self._check(self._lib.mppi_set_nominal_control(self._h, u))

    def injectNoise(self, eps):
        """eps[n_iters][K_local][T][C] (or [K_local][T][C]); None switches back to the generator."""
        if eps is None:
            self._check(self._lib.mppi_inject_noise(self._h, None, 0))
            return
        eps = _f32(eps)
        if eps.ndim == len(self._noise_shape()):
            eps = eps[None]
        assert eps.shape[1:] == self._noise_shape(), (eps.shape, self._noise_shape())
        self._check(self._lib.mppi_inject_noise(self._h, eps.ctypes.data, eps.shape[0]))

    def _noise_shape(self):
        if getattr(self, "sampler", MPPI_SAMPLER_GAUSSIAN) == MPPI_SAMPLER_COLORED:
            # spectrum noise, the reference's samples_in_freq_complex_d_ layout: [K][C][T+1][2], one spectrum for every system
            return (self.num_rollouts_local, self.CONTROL_DIM, self.num_timesteps + 1, 2)
        base = (self.num_rollouts_local, self.num_timesteps, self.CONTROL_DIM)
        return ((self.num_systems,) + base) if getattr(self, "_independent_noise", False) else base

    def setColoredNoiseParams(self, exponents, offset_decay_rate=0.97, fmin=0.0):
        """ColoredNoiseParams of a handle whose sampler is the colored-noise one (ColoredMPPIController, or
        TubeMPPIController(..., sampler=MPPI_SAMPLER_COLORED)); MPPIError(MPPI_ERR_STATE) on any other"""
        self._check(self._lib.mppi_set_colored_noise_params(self._h, _f32(exponents).reshape(-1), offset_decay_rate, fmin))

    def setIndependentNoise(self, independent=True):
        """use_same_noise_for_all_distributions = not independent (sampling_distribution.cuh:20); injected noise then is
        eps[n_iters][D][K_local][T][C]"""
        self._check(self._lib.mppi_set_independent_noise(self._h, int(independent)))
        self._independent_noise = bool(independent)

    def sampleNoise(self, optimization_stride=1):
        """raw eps[K_local][T][C] of the next iteration (generator tests; see mppi_sample_noise)"""
        eps = np.empty((self.num_rollouts_local, self.num_timesteps, self.CONTROL_DIM), np.float32)
        self._check(self._lib.mppi_sample_noise(self._h, optimization_stride, eps))
        return eps

    def computeControl(self, state, optimization_stride=1):
        """state: the measured state, STATE_DIM floats for every controller (mppi_compute_control reads exactly that many:
        Tube and Robust MPPI keep their nominal state themselves); any other size raises MPPIError(MPPI_ERR_INVALID_ARG)"""
        if type(state) is not np.ndarray:
            state = np.asarray(state, np.float32)
        self._check_state_size(state, "computeControl")
        self._x_stage[:] = state if state.ndim == 1 else state.reshape(-1)
        st = self._fast_compute(self._hv, self._x_ptr, optimization_stride)
        if st != 0:
            self._check(st)

    def _check_state_size(self, state, what):
        """the library reads exactly STATE_DIM floats of a measured state: any other size is the caller's error"""
        if np.size(state) != self.STATE_DIM:
            raise MPPIError(MPPI_ERR_INVALID_ARG, "%s: a state of %d floats, the model's state has %d"
                            % (what, np.size(state), self.STATE_DIM))

    def getControlSeq(self):
        st = self._fast_get_control(self._hv, self._u_ptr)
        if st != 0:
            self._check(st)
        return self._u_stage.copy()

    def getTargetStateSeq(self):
        x = np.empty((self.num_timesteps, self.STATE_DIM), np.float32)
        self._check(self._lib.mppi_get_state_seq(self._h, x))
        return x

    def hasComputeGrad(self):
        """does the model's Dynamics class declare a device computeGrad (mppi_has_compute_grad)"""
        return bool(self._lib.mppi_has_compute_grad(self._h))

    def computeGrad(self, states, controls):
        """Dynamics::computeGrad at n points: states (n, S) and controls (n, C) (one point may be given flat) -> the
        continuous-time Jacobians A (n, S, S) = d xdot / d x and B (n, S, C) = d xdot / d u, float32 (mppi_linearize)"""
        x = np.ascontiguousarray(states, np.float32).reshape(-1, self.STATE_DIM)
        u = np.ascontiguousarray(controls, np.float32).reshape(-1, self.CONTROL_DIM)
        if x.shape[0] != u.shape[0]:
            raise MPPIError(MPPI_ERR_INVALID_ARG, "computeGrad: %d states, %d controls" % (x.shape[0], u.shape[0]))
        n = x.shape[0]
        A = np.empty((n, self.STATE_DIM, self.STATE_DIM), np.float32)
        B = np.empty((n, self.STATE_DIM, self.CONTROL_DIM), np.float32)
        self._check(self._lib.mppi_linearize(self._h, x.reshape(-1), u.reshape(-1), n, A.reshape(-1), B.reshape(-1)))
        return A, B

    def computeGradTrajectory(self, system=0):
        """A (T, S, S), B (T, S, C) along the result of the last computeControl, read on the device
        (mppi_linearize_trajectory): system 0 the sequences getTargetStateSeq / getControlSeq return, system 1 the nominal
        ones of a Tube / Robust controller"""
        A = np.empty((self.num_timesteps, self.STATE_DIM, self.STATE_DIM), np.float32)
        B = np.empty((self.num_timesteps, self.STATE_DIM, self.CONTROL_DIM), np.float32)
        self._check(self._lib.mppi_linearize_trajectory(self._h, system, A.reshape(-1), B.reshape(-1)))
        return A, B

    def setFeedbackParams(self, Q=None, R=None, Q_f=None, num_iterations=1):
        """DDPParams of the tracking controller (mppi_set_feedback_params): Q (S, S), R (C, C), Q_f (S, S); None is the identity,
        the DDPParams default.  num_iterations other than 1 raises MPPIError(MPPI_ERR_UNSUPPORTED)."""
        def mat(m, n, name):
            if m is None:
                return None, None
            a = np.ascontiguousarray(m, np.float32)
            if a.shape != (n, n):
                raise MPPIError(MPPI_ERR_INVALID_ARG, "setFeedbackParams: %s is %s, expected (%d, %d)" % (name, a.shape, n, n))
            return a, a.ctypes.data
        q, qp = mat(Q, self.STATE_DIM, "Q")
        r, rp = mat(R, self.CONTROL_DIM, "R")
        f, fp = mat(Q_f, self.STATE_DIM, "Q_f")
        self._check(self._lib.mppi_set_feedback_params(self._h, qp, rp, fp, int(num_iterations)))

    def computeFeedback(self, system=0):
        """the DDP tracking gains (T, S, C), [t][i][j] = K_t(j, i), along the result of the last computeControl, linearised and
        solved on the device (mppi_compute_feedback): system 0 the sequences getTargetStateSeq / getControlSeq return, system 1
        the nominal ones of a Tube / Robust controller — a Robust controller also installs that result as its gains"""
        g = np.empty((self.num_timesteps, self.STATE_DIM, self.CONTROL_DIM), np.float32)
        self._check(self._lib.mppi_compute_feedback(self._h, int(system), g.ctypes.data))
        return g

    def computeFeedbackAt(self, states, controls):
        """the same at the caller's points, states (T, S) and controls (T, C) (mppi_compute_feedback_at); installs nothing"""
        x = np.ascontiguousarray(states, np.float32).reshape(-1)
        u = np.ascontiguousarray(controls, np.float32).reshape(-1)
        if x.size != self.num_timesteps * self.STATE_DIM or u.size != self.num_timesteps * self.CONTROL_DIM:
            raise MPPIError(MPPI_ERR_INVALID_ARG, "computeFeedbackAt: states (%d, %d) and controls (%d, %d) expected"
                            % (self.num_timesteps, self.STATE_DIM, self.num_timesteps, self.CONTROL_DIM))
        g = np.empty((self.num_timesteps, self.STATE_DIM, self.CONTROL_DIM), np.float32)
        self._check(self._lib.mppi_compute_feedback_at(self._h, x.ctypes.data, u.ctypes.data, g.ctypes.data))
        return g

    def getTargetOutputSeq(self):
        y = np.empty((self.num_timesteps, self.OUTPUT_DIM), np.float32)
        self._check(self._lib.mppi_get_output_seq(self._h, y))
        return y

    def slideControlSequence(self, steps):
        st = self._fast_slide(self._hv, steps)
        if st != 0:
            self._check(st)

    def getSampledCostSeq(self):
        costs = np.empty((self.num_systems, self.num_rollouts_local), np.float32)
        self._check(self._lib.mppi_get_costs(self._h, costs))
        return costs

    def getSampledControls(self):
        v = np.empty((self.num_systems, self.num_rollouts_local, self.num_timesteps, self.CONTROL_DIM), np.float32)
        self._check(self._lib.mppi_get_sampled_controls(self._h, v))
        return v

    def top_rollouts(self, n, system=0):
        """(indices, costs) of the n lowest-cost local rollouts of the last iteration, selected on the device
        (mppi_top_rollouts): ascending cost, ties to the lower index, NaN last; costs as getSampledCostSeq gives them"""
        n = int(n)
        idx = np.empty(max(n, 0), np.int32)
        cost = np.empty(max(n, 0), np.float32)
        self._check(self._lib.mppi_top_rollouts(self._h, int(system), n, idx.ctypes.data, cost.ctypes.data))
        return idx, cost

    def replay_rollouts(self, indices, system=0):
        """the rows `indices` (local rollout indices of the saved samples; -1: the current control sequence) run again on the
        device (mppi_replay_rollouts): (outputs (n, T, O) after each step, step costs (n, T + 1) with the terminal cost last,
        crash flags (n, T))"""
        idx = np.ascontiguousarray(np.asarray(indices).reshape(-1), np.int32)
        n, T = idx.size, self.num_timesteps
        y = np.empty((n, T, self.OUTPUT_DIM), np.float32)
        cost = np.empty((n, T + 1), np.float32)
        crash = np.empty((n, T), np.int32)
        self._check(self._lib.mppi_replay_rollouts(self._h, int(system), idx.ctypes.data, n, y.ctypes.data, cost.ctypes.data,
                                                   crash.ctypes.data))
        return y, cost, crash

    def _control_rows(self, u, what):
        u = np.ascontiguousarray(u, np.float32)
        row = self.num_timesteps * self.CONTROL_DIM
        if u.size % row != 0:
            raise MPPIError(MPPI_ERR_INVALID_ARG, "%s: control sequences of shape (n, %d, %d) expected, got %s"
                            % (what, self.num_timesteps, self.CONTROL_DIM, u.shape))
        return u.reshape(-1, self.num_timesteps, self.CONTROL_DIM)

    def evaluate_controls(self, x0, u):
        """(costs (n,), crash flags (n,)) of the caller's control sequences u (n, T, C) rolled out on the device from x0 (S,) — one
        initial state for every row — or x0 (n, S), one per row (mppi_evaluate_controls): the rollout kernel's trajectory cost of
        a rollout whose clamped controls are u[i], without the likelihood-ratio term (a candidate is no sample of the current
        distribution), and the crash status after the last step.  Nothing the controller computes depends on the call."""
        u = self._control_rows(u, "evaluate_controls")
        x = np.ascontiguousarray(x0, np.float32)
        if x.size % self.STATE_DIM != 0:
            raise MPPIError(MPPI_ERR_INVALID_ARG, "evaluate_controls: initial states of %d floats expected, got %s"
                            % (self.STATE_DIM, x.shape))
        n = u.shape[0]
        cost = np.empty(n, np.float32)
        crash = np.empty(n, np.int32)
        self._check(self._lib.mppi_evaluate_controls(self._h, x.ctypes.data, x.size // self.STATE_DIM, u.ctypes.data, n,
                                                     cost.ctypes.data, crash.ctypes.data))
        return cost, crash

    def warm_start(self, x0, candidates, hysteresis=0.0):
        """(chosen, costs (n + 1,)): the current control sequence (getControlSeq) and the candidates (n, T, C) evaluated from x0 in
        one launch (mppi_warm_start); the cheapest candidate is installed as setNominalControl would install it if its cost is
        below current - hysteresis, or if the current cost is NaN and its own is not.  chosen is its index, or -1 when the
        current sequence stays; costs[0] is the current sequence's cost.  Vanilla, Colored and Tube controllers."""
        self._check_state_size(x0, "warm_start")
        u = self._control_rows(candidates, "warm_start")
        x = _f32(x0).reshape(-1)
        n = u.shape[0]
        chosen = C.c_int(-1)
        cost = np.empty(n + 1, np.float32)
        self._check(self._lib.mppi_warm_start(self._h, x.ctypes.data, u.ctypes.data, n, float(hysteresis),
                                              C.addressof(chosen), cost.ctypes.data))
        return chosen.value, cost

    def sampled_trajectories(self, top_n=0, fraction=0.0, seed=None, system=0):
        """the reference's calculateSampledStateTrajectories (controllers/controller.cu:55-179): replays slot 0 = the optimal
        sequence, then int(fraction * K) rollouts drawn without replacement from the first 98 % of the local rollouts (the last
        ones are pure noise) with a seeded host generator, then the top_n lowest-cost rollouts.  Returns a dict: "indices" (the
        list, -1 first), "outputs", "costs", "crash" (replay_rollouts of it) and "top_costs" (top_n costs, ascending)."""
        idx = sampled_trajectory_list(self.num_rollouts_local, fraction, seed)
        top_costs = np.empty(0, np.float32)
        if top_n > 0:
            top_idx, top_costs = self.top_rollouts(top_n, system)
            idx = np.concatenate([idx, top_idx])
        y, cost, crash = self.replay_rollouts(idx, system)
        return {"indices": idx, "outputs": y, "costs": cost, "crash": crash, "top_costs": top_costs}

    def getStats(self):
        st = MppiStats()
        self._check(self._lib.mppi_get_stats(self._h, C.byref(st)))
        return st

    def getBaselineCost(self, system=0):
        st = self.getStats()
        return (st.real_sys if system == 0 else st.nominal_sys).baseline

    def getNormalizerCost(self, system=0):
        st = self.getStats()
        return (st.real_sys if system == 0 else st.nominal_sys).normalizer

    # -- kernel-level / device-resident --
    def rolloutCosts(self, x0, optimization_stride=1):
        self._check(self._lib.mppi_rollout_costs(self._h, _f32(x0).reshape(-1), optimization_stride))
        return self.getSampledCostSeq()

    def uploadState(self, x0):
        self._check(self._lib.mppi_upload_state(self._h, _f32(x0).reshape(-1)))

    def getOptimalControlSeq(self):
        """raw u* of the last iteration ([D][T][C]); reference: setHostOptimalControlSequence"""
        u = np.empty((self.num_systems, self.num_timesteps, self.CONTROL_DIM), np.float32)
        self._check(self._lib.mppi_get_optimal_control(self._h, u))
        return u

    def optimize(self, num_iterations, synchronize=True):
        self._check(self._lib.mppi_optimize(self._h, num_iterations, int(synchronize)))

    def timeIterations(self, n):
        a, b = C.c_float(), C.c_float()
        self._check(self._lib.mppi_time_iterations(self._h, n, C.byref(a), C.byref(b)))
        return a.value, b.value

    def synchronize(self):
        self._check(self._lib.mppi_synchronize(self._h))

    def chooseAppropriateKernel(self, num_evaluations=10):
        """times the fused and the role-pipelined rollout kernel and keeps the faster (mppi_controller.cu:44-143);
        returns (variant, fused_ms, pipeline_ms) with variant 1 = fused, 2 = pipeline"""
        v, a, b = C.c_int(), C.c_float(), C.c_float()
        self._check(self._lib.mppi_choose_kernel(self._h, num_evaluations, C.byref(v), C.byref(a), C.byref(b)))
        return v.value, a.value, b.value

    def enforceConstraints(self, state, u):
        """Dynamics::enforceConstraints on one control vector (host-side and lock-free for the base rule)"""
        u = _f32(u).reshape(-1).copy()
        sp = None if state is None else _f32(state).reshape(-1).ctypes.data
        self._check(self._lib.mppi_enforce_constraints(self._h, sp, u))
        return u

    def modelStep(self, x, u, dt=None, enforce_constraints=True):
        x = _f32(x).reshape(-1).copy()
        u = _f32(u).reshape(-1).copy()
        self._check(self._lib.mppi_model_step(self._h, x, u, self.dt if dt is None else dt, int(enforce_constraints)))
        return x, u

    # -- multi-GPU --
    def exchangeBuffers(self):
        s, r, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
        self._check(self._lib.mppi_get_exchange_buffers(self._h, C.byref(s), C.byref(r), C.byref(n)))
        return s.value, r.value, n.value

    def readSendRecord(self):
        n = self.exchangeBuffers()[2]
        out = np.empty(n, np.float32)
        self._check(self._lib.mppi_read_send_record(self._h, out))
        return out

    def writeRecvRecords(self, records):
        r = _f32(records).reshape(-1)
        self._check(self._lib.mppi_write_recv_records(self._h, r))

    def iterationLocal(self):
        self._check(self._lib.mppi_iteration_local(self._h))

    def iterationMerge(self):
        self._check(self._lib.mppi_iteration_merge(self._h))

    def p2pMailboxHandle(self):
        """64-byte hipIpcMemHandle_t of this rank's mailbox (to be exchanged between the processes)"""
        buf = C.create_string_buffer(64)
        n = C.c_size_t()
        self._check(self._lib.mppi_p2p_mailbox_handle(self._h, buf, 64, C.byref(n)))
        return bytes(buf.raw[:n.value])

    def p2pReset(self):
        """ends this rank's mailbox session (mppi_p2p_reset): every rank calls it before a NEW session exports / connects"""
        self._check(self._lib.mppi_p2p_reset(self._h))

    def p2pConnect(self, handles):
        """handles: list of world byte strings (rank order) from p2pMailboxHandle of every rank"""
        blob = b"".join(h.ljust(64, b"\0") for h in handles)
        self._check(self._lib.mppi_p2p_connect(self._h, blob, 64))

    @staticmethod
    def p2pConnectLocal(controllers):
        """all ranks of one problem living in this process: wire their mailboxes together"""
        arr = (C.c_void_p * len(controllers))(*[c._h.value for c in controllers])
        for c in controllers:
            c._check(c._lib.mppi_p2p_connect_local(c._h, arr))

    def commInitRccl(self, unique_id_bytes):
        buf = C.create_string_buffer(bytes(unique_id_bytes), 128)
        self._check(self._lib.mppi_comm_init_rccl(self._h, buf, 128))


class VanillaMPPIController(MPPIController):
    """reference: controllers/MPPI/mppi_controller.cuh — VanillaMPPIController"""
    KIND = MPPI_CONTROLLER_VANILLA


class ColoredMPPIController(MPPIController):
    """reference: controllers/ColoredMPPI/colored_mppi_controller.cuh — ColoredMPPIController with
    ColoredNoiseDistribution (sampling_distributions/colored_noise/colored_noise.cuh)"""
    KIND = MPPI_CONTROLLER_COLORED

    def setColoredMPPIParams(self, gamma=0.0, r_exp=0.0, state_leash_dist=None, leash_active=False, leash_jump=1):
        """setGamma / setRExp (Tsallis weights when both are non-zero) and the state leash (setStateLeashLength,
        setLeashActive; colored_mppi_controller.cuh:95-193)"""
        p = None if state_leash_dist is None else _f32(state_leash_dist).reshape(-1).ctypes.data
        self._check(self._lib.mppi_set_colored_mppi_params(self._h, gamma, r_exp, p, int(leash_active), leash_jump))


class RobustMPPIController(MPPIController):
    """reference: controllers/R-MPPI/robust_mppi_controller.cuh — RobustMPPIController.
    Systems: 0 = nominal, 1 = real.  The DDP gains come from the caller (setFeedbackGains) or from computeFeedback(system=1)."""
    KIND = MPPI_CONTROLLER_ROBUST

    def setRMPPIParams(self, value_function_threshold=1000.0, num_candidates=9, samples_per_candidate=32):
        self.num_candidates = num_candidates
        self._check(self._lib.mppi_set_rmppi_params(self._h, value_function_threshold, num_candidates,
                                                    samples_per_candidate))

    def setFeedbackGains(self, gains, accumulate_all_states=False):
        """gains[T][S][C] (DDPFeedbackState::fb_gain_traj_)"""
        g = _f32(gains)
        assert g.shape == (self.num_timesteps, self.STATE_DIM, self.CONTROL_DIM), g.shape
        self._check(self._lib.mppi_set_feedback_gains(self._h, g.reshape(-1), int(accumulate_all_states)))

    def updateImportanceSamplingControl(self, state, stride):
        """state: the measured state, STATE_DIM floats; any other size raises MPPIError(MPPI_ERR_INVALID_ARG)"""
        self._check_state_size(state, "updateImportanceSamplingControl")
        self._check(self._lib.mppi_update_importance_sampling_control(self._h, _f32(state).reshape(-1), stride))

    def getRMPPIState(self):
        """(nominal_state[S], best_index, nominal_stride, candidate_free_energy[num_candidates])"""
        ns = np.zeros(self.STATE_DIM, np.float32)
        fe = np.zeros(getattr(self, "num_candidates", 9), np.float32)
        bi, st = C.c_int(), C.c_int()
        self._check(self._lib.mppi_get_rmppi_state(self._h, ns.ctypes.data, C.byref(bi), C.byref(st), fe.ctypes.data))
        return ns, bi.value, st.value, fe

    def getNominalControlSeq(self):
        u = np.empty((self.num_timesteps, self.CONTROL_DIM), np.float32)
        self._check(self._lib.mppi_get_nominal_control_seq(self._h, u))
        return u

    def getNominalStateSeq(self):
        x = np.empty((self.num_timesteps, self.STATE_DIM), np.float32)
        self._check(self._lib.mppi_get_nominal_state_seq(self._h, x))
        return x


class TubeMPPIController(MPPIController):
    """reference: controllers/Tube-MPPI/tube_mppi_controller.cuh — TubeMPPIController"""
    KIND = MPPI_CONTROLLER_TUBE

    def setNominalThreshold(self, t):
        self._check(self._lib.mppi_set_nominal_threshold(self._h, t))

    def getNominalControlSeq(self):
        u = np.empty((self.num_timesteps, self.CONTROL_DIM), np.float32)
        self._check(self._lib.mppi_get_nominal_control_seq(self._h, u))
        return u

    def getNominalStateSeq(self):
        x = np.empty((self.num_timesteps, self.STATE_DIM), np.float32)
        self._check(self._lib.mppi_get_nominal_state_seq(self._h, x))
        return x


# ---- introspection --------------------------------------------------------------------------------------------------
# mppi_kernel_family (include/mppi_amd.h), by value
KERNEL_FAMILIES = ("none", "fused", "fused_rep", "pipeline", "pipeline_fold", "pipeline_rep", "rmppi", "rmppi_pipeline")
MPPI_SAMPLER_GAUSSIAN = 0
MPPI_SAMPLER_COLORED = 1
MPPI_SAMPLER_NLN = 2
MPPI_SAMPLER_COLORED_TUBE = 3  # a registry key (describe_model): the two-system colored instantiation Tube runs
_MODEL_CAPS = (("pipeline", 1), ("rmppi", 2), ("rmppi_pipeline", 4), ("rows_in_hbm", 8), ("streamed_merge", 16),
               ("pipeline_fold", 32))


def list_models():
    """names of the registered instantiations (mppi_list_models)"""
    return [n for n in load_library().mppi_list_models().decode().split("\n") if n]


def describe_model(name, sampler_kind=MPPI_SAMPLER_GAUSSIAN):
    """what a registered (model, sampler) instantiation offers, without a device (mppi_describe_model): dict with "shapes"
    (every registered (bx, by, bz)), "replicated_lane_shapes" (those that run the replicated-lane dynamics form) and one bool
    per capability ("pipeline", "rmppi", "rmppi_pipeline", "rows_in_hbm", "streamed_merge", "pipeline_fold"); None when the
    model has no instantiation for that sampler"""
    lib = load_library()
    n, caps = C.c_int(), C.c_uint()
    st = lib.mppi_describe_model(name.encode(), sampler_kind, None, 0, C.byref(n), C.byref(caps))
    if st == MPPI_ERR_UNKNOWN_MODEL:
        return None
    _op_check(lib, st)
    buf = (C.c_int * (4 * n.value))()
    _op_check(lib, lib.mppi_describe_model(name.encode(), sampler_kind, buf, n.value, C.byref(n), C.byref(caps)))
    rows = [tuple(buf[4 * i:4 * i + 4]) for i in range(n.value)]
    d = {"shapes": [r[:3] for r in rows], "replicated_lane_shapes": [r[:3] for r in rows if r[3]]}
    d.update({k: bool(caps.value & bit) for k, bit in _MODEL_CAPS})
    return d


# ---- kernel-level operators -----------------------------------------------------------------------------------------
def _op_check(lib, st):
    if st != 0:
        raise MPPIError(st, (lib.mppi_last_error(None) or b"").decode())


def npz_read_array(path, key):
    """one array of an .npz through the library's own reader (host only; returns float64 in C order)"""
    lib = load_library()
    n, nd = C.c_size_t(), C.c_int()
    dims = (C.c_int * 8)()
    _op_check(lib, lib.mppi_npz_read_array(str(path).encode(), key.encode(), None, 0, C.byref(n), dims, C.byref(nd)))
    out = np.empty(n.value, np.float64)
    _op_check(lib, lib.mppi_npz_read_array(str(path).encode(), key.encode(), out.ctypes.data, n.value, C.byref(n), dims,
                                           C.byref(nd)))
    return out.reshape([dims[i] for i in range(nd.value)])


def texture2d_query(data, points, frame, params=None, device=0):
    """TwoDTextureHelper lookups on the device (mppi_texture2d_query): data[h][w] or [h][w][channels], points[n][3],
    frame 0 texture coordinate / 1 map pose / 2 world pose"""
    from .capi import MppiTexture2dParams
    lib = load_library()
    d = _f32(data)
    if d.ndim == 2:
        d = d[:, :, None]
    h, w, ch = d.shape
    pts = _f32(points).reshape(-1, 3)
    out = np.zeros((pts.shape[0], ch), np.float32)
    p = params if params is not None else MppiTexture2dParams()
    _op_check(lib, lib.mppi_texture2d_query(d.reshape(-1), w, h, ch, C.byref(p), pts.reshape(-1), pts.shape[0], frame,
                                            out.reshape(-1), device))
    return out


class LSTMLSTMHelper:
    """Host side of the reference's LSTMLSTMHelper (utils/nn_helpers/lstm_lstm_helper.cuh; C++ in
    include/mppi_amd/utils/nn_helpers/lstm_lstm_helper.hpp): the initialiser LSTM that turns the recent history buffer into
    the initial (hidden, cell) of the prediction LSTM inside the rollouts.  initializeLSTM() returns them; hand them to
    controller.setLSTMInitialState()."""

    def __init__(self, init_input_dim, init_hidden_dim, init_output_layers, input_dim, hidden_dim, output_layers, init_len):
        assert init_output_layers[0] == init_input_dim + init_hidden_dim and init_output_layers[-1] == 2 * hidden_dim
        self.init_input_dim, self.init_hidden_dim = init_input_dim, init_hidden_dim
        self.init_output_layers = list(init_output_layers)
        self.input_dim, self.hidden_dim, self.output_layers, self.init_len = input_dim, hidden_dim, list(output_layers), init_len
        H, I = init_hidden_dim, init_input_dim
        self.init_lstm = np.zeros(4 * H * H + 4 * H * I + 6 * H, np.float32)
        n = sum(self.init_output_layers[i + 1] * (self.init_output_layers[i] + 1) for i in range(len(init_output_layers) - 1))
        self.init_output = np.zeros(n, np.float32)

    def setInitParams(self, lstm_blob, output_blob):
        """initialiser parameters in the device helpers' blob layouts (lstm_blob_from_npz_dict(d, "init_") builds them)"""
        lstm_blob, output_blob = _f32(lstm_blob).reshape(-1), _f32(output_blob).reshape(-1)
        assert lstm_blob.size == self.init_lstm.size and output_blob.size == self.init_output.size
        self.init_lstm, self.init_output = lstm_blob.copy(), output_blob.copy()

    def initializeLSTM(self, buffer):
        """buffer[init_input_dim][cols] as the reference's Eigen matrix (one column per time step); returns (hidden, cell)"""
        buffer = _f32(buffer)
        if buffer.ndim != 2 or buffer.shape[0] != self.init_input_dim or buffer.shape[1] < self.init_len:
            raise ValueError("history buffer must be [init_input_dim][>= init_len]")
        lib = load_library()
        cols = buffer.shape[1]
        samples = np.ascontiguousarray(buffer.T).reshape(-1)
        out = np.zeros(2 * self.hidden_dim, np.float32)
        layers = (C.c_int * len(self.init_output_layers))(*self.init_output_layers)
        _op_check(lib, lib.mppi_lstm_lstm_initialize(self.init_input_dim, self.init_hidden_dim, layers,
                                                     len(self.init_output_layers), self.init_lstm, self.init_output,
                                                     self.hidden_dim, self.init_len, samples, cols, out))
        return out[:self.hidden_dim].copy(), out[self.hidden_dim:].copy()


def det_eval(func, x, device=0):
    lib = load_library()
    x = _f32(x).reshape(-1)
    y = np.empty_like(x)
    _op_check(lib, lib.mppi_det_eval(func, x, y, x.size, device))
    return y


def det_atan2(y, x, device=0):
    """det::atan2 on the device (mppi_det_eval function 14, which takes its arguments as (y, x) pairs)"""
    y, x = np.broadcast_arrays(_f32(y), _f32(x))
    pairs = np.stack([y.reshape(-1), x.reshape(-1)], axis=1)
    return det_eval(14, pairs, device)[0::2].reshape(y.shape)


def launch_boundary_us(device=0, n=2000):
    """average time per launch of n dependent trivial kernels (mppi_measure_launch_boundary)"""
    lib = load_library()
    out = C.c_float()
    _op_check(lib, lib.mppi_measure_launch_boundary(device, n, C.byref(out)))
    return float(out.value)


def issue_interval_ns(device=0):
    """ns per dependent 4-byte VALU instruction of a wave alone on its SIMD (mppi_measure_issue_interval)"""
    lib = load_library()
    out = C.c_float()
    _op_check(lib, lib.mppi_measure_issue_interval(device, C.byref(out)))
    return float(out.value)


def philox_normal(seed, generation, K, T, Cdim, k_begin=0, k_end=None, device=0):
    lib = load_library()
    k_end = K if k_end is None else k_end
    out = np.empty((k_end - k_begin, T, Cdim), np.float32)
    _op_check(lib, lib.mppi_philox_normal(seed, generation, K, T, Cdim, k_begin, k_end, out, device))
    return out


def norm_exp(costs, lambda_inv, baseline, device=0):
    lib = load_library()
    w = _f32(costs).reshape(-1).copy()
    _op_check(lib, lib.mppi_norm_exp(w, w.size, lambda_inv, baseline, device))
    return w


def compute_weights(costs, lambda_inv, device=0):
    lib = load_library()
    w = _f32(costs).reshape(-1).copy()
    out = np.zeros(2, np.float32)
    _op_check(lib, lib.mppi_compute_weights(w, w.size, lambda_inv, out, device))
    return w, float(out[0]), float(out[1])


def compute_weights_reference_order(costs, lambda_, device=0):
    """weights, stats8 = {rho, eta, free energy mean / variance / modified variance, sum w^2, 0, 0} in the reference's order"""
    lib = load_library()
    w = _f32(costs).reshape(-1).copy()
    st = np.zeros(8, np.float32)
    _op_check(lib, lib.mppi_compute_weights_reference_order(w, w.size, lambda_, st, device))
    return w, st


def weighted_reduction_reference_order(weights, v, normalizer, sum_stride=32, fma=False, device=0):
    lib = load_library()
    v = _f32(v)
    K, T, Cd = v.shape
    u = np.empty((T, Cd), np.float32)
    _op_check(lib, lib.mppi_weighted_reduction_reference_order(_f32(weights).reshape(-1), v, normalizer, K, T, Cd,
                                                               sum_stride, 1 if fma else 0, u, device))
    return u


def weighted_reduction(weights, v, normalizer, device=0):
    lib = load_library()
    v = _f32(v)
    K, T, Cd = v.shape
    u = np.empty((T, Cd), np.float32)
    _op_check(lib, lib.mppi_weighted_reduction(_f32(weights).reshape(-1), v, normalizer, K, T, Cd, u, device))
    return u
