"""The RACER Dubins family's synthetic configurations (elevation map, LSTM steering, suspension, uncertainty networks), built
identically for the HIP engine and the CPU oracle as the cfg dicts of common.py, with the state and output indices and the
float64 suspension restatement that several test files share.  The tests of each model are in tests/test_racer_dubins_*.py."""
import math

import numpy as np

import mppi_generic_amd as m

# states of the suspension (the first 13, 24 in all) and the uncertainty model (26 in all); the elevation and LSTM-steering
# models (19 states) share 0..7 and keep STEER_ANGLE_RATE at 8
(S_VEL, S_YAW, S_X, S_Y, S_STEER, S_BRAKE, S_ROLL, S_PITCH, S_CGZ, S_CGVZ, S_ROLL_RATE, S_PITCH_RATE, S_STEER_RATE, S_OMEGA,
 S_STATIC_ROLL, S_STATIC_PITCH) = range(16)
ELEVATION_S_STEER_RATE = 8
O_POS_Z, O_F_UP, O_F_FWD, O_F_SIDE = 4, 10, 11, 12
NS_SUSPENSION = 24
WHEELS = [(2.981, 0.737), (2.981, -0.737), (0.0, -0.737), (0.0, 0.737)]   # FL, FR, BL, BR as the reference places them
UNC = 16   # UNCERTAINTY_POS_X, _POS_Y, _YAW, _VEL_X, _POS_X_Y, _POS_X_YAW, _POS_X_VEL_X, _POS_Y_YAW, _POS_Y_VEL_X, _YAW_VEL_X
NS_UNCERTAINTY = 26
MEAN_LSTM, MEAN_OUT = 4 * 16 + 4 * 4 * 12 + 16 + 8, 20 * 16 + 20 + 2 * 20 + 2
UNC_LSTM, UNC_OUT = 4 * 16 + 4 * 4 * 13 + 16 + 8, 20 * 17 + 20 + 5 * 20 + 5
H, I = 4, 4
LSTM_PARAMS = 4 * H * H + 4 * H * I + 4 * H
OUT_LAYERS = [8, 20, 1]
OUT_PARAMS = 8 * 20 + 20 + 20 * 1 + 1


# a state of the 19-, 24- and 26-state models from its leading entries: st, st24, st26
def st(*v):
    x = np.zeros(19, np.float32)
    x[:len(v)] = v
    return x


def hills(n=240, res=0.25):
    """a smooth synthetic terrain, (blob, transform); world window [-30, 30]^2"""
    c = (np.arange(n) + 0.5) * res - 30.0
    X, Y = np.meshgrid(c, c)
    z = 0.8 * np.sin(0.21 * X) * np.cos(0.17 * Y) + 0.03 * X + 0.4 * np.exp(-((X - 6) ** 2 + (Y - 3) ** 2) / 18.0)
    transform = np.array([-30.0, -30.0, 0.0, 1, 0, 0, 0, 1, 0, 0, 0, 1, res, res, 1.0], np.float32)
    return z.astype(np.float32), transform


def elevation_cfg(K=1024, T=60, lambda_=0.5, num_iters=1, D=1, with_map=True):
    """drive towards a way-point at 3 m/s over the hills, keeping the position variance small; outputs the model does not
    produce (NaN) carry coefficient 0"""
    cost = m.QuadraticCostParams28()
    coeffs, goal = [0.0] * 28, [0.0] * 28
    coeffs[0], goal[0] = 20.0, 3.0   # BASELINK_VEL_B_X
    coeffs[2], goal[2] = 1.0, 8.0    # BASELINK_POS_I_X
    coeffs[3], goal[3] = 1.0, 3.0    # BASELINK_POS_I_Y
    coeffs[6] = 30.0                 # ROLL
    coeffs[7] = 10.0                 # PITCH
    coeffs[9] = 0.05                 # STEER_ANGLE_RATE
    coeffs[17] = coeffs[18] = 5.0    # UNCERTAINTY_POS_X / _Y
    cost.s_coeffs[:] = coeffs
    cost.s_goal[:] = goal
    x0 = np.zeros(19, np.float32)
    x0[:9] = [1.0, 0.2, -4.0, -2.0, 0.03, 0.0, 0.0, 0.0, 0.0]
    x0[9:13] = [0.01, 0.01, 0.001, 0.02]
    cfg = dict(model="racer_dubins_elevation", K=K, T=T, D=D, dt=0.05, lambda_=lambda_, alpha=0.0, num_iters=num_iters,
               dyn=m.RacerDubinsElevationParams(), cost=cost, ranges=[-1.0, 1.0, -1.0, 1.0], std_dev=[0.4, 0.5],
               control_cost_coeff=[0.0, 0.0], x0=x0)
    b = cfg["dyn"].base   # a drivable car: 5 m/s^2 at full throttle, drag 1/s, brakes 5 m/s^2 per 0.25 of brake state
    b.c_0 = 0.0
    b.c_t[:] = [5.0, 5.0, 5.0]
    b.c_v[:] = [1.0, 1.0, 1.0]
    b.c_b[:] = [20.0, 20.0, 20.0]
    b.wheel_base = 2.981
    b.steer_angle_scale = -2.45
    if with_map:
        heights, transform = hills()
        cfg["blobs"] = {"elevation_map": heights, "elevation_map_transform": transform}
    return cfg


def steering_blobs(seed=21, scale=0.4, zero=False):
    rng = np.random.default_rng(seed)
    lstm = np.zeros(LSTM_PARAMS + 2 * H, np.float32) if zero else rng.uniform(-scale, scale, LSTM_PARAMS + 2 * H).astype(np.float32)
    out = np.zeros(OUT_PARAMS, np.float32) if zero else rng.uniform(-scale, scale, OUT_PARAMS).astype(np.float32)
    return {"lstm_weights": lstm, "lstm_output_weights": out}


def steering_cfg(zero=False, **kw):
    cfg = elevation_cfg(**kw)
    cfg["model"] = "racer_dubins_elevation_lstm_steering"
    blobs = dict(cfg.get("blobs", {}))
    blobs.update(steering_blobs(zero=zero))
    cfg["blobs"] = blobs
    return cfg


def st24(*v):
    x = np.zeros(NS_SUSPENSION, np.float32)
    x[:len(v)] = v
    return x


def normals_of(z, res):
    """unit normals of a height field z[row = y][col = x] sampled every `res` metres: {h, w, 4}"""
    dzdy, dzdx = np.gradient(z.astype(np.float64), res)
    n = np.stack([-dzdx, -dzdy, np.ones_like(dzdx), np.zeros_like(dzdx)], axis=-1)
    n[..., :3] /= np.linalg.norm(n[..., :3], axis=-1, keepdims=True)
    return n.astype(np.float32)


def suspension_cfg(K=1024, T=60, lambda_=0.5, D=1, maps="both", zero_net=False):
    cost = m.QuadraticCostParams28()
    coeffs, goal = [0.0] * 28, [0.0] * 28
    coeffs[0], goal[0] = 20.0, 3.0   # BASELINK_VEL_B_X
    coeffs[2], goal[2] = 1.0, 8.0    # BASELINK_POS_I_X
    coeffs[3], goal[3] = 1.0, 3.0    # BASELINK_POS_I_Y
    coeffs[6] = 30.0                 # ROLL
    coeffs[7] = 10.0                 # PITCH
    coeffs[9] = 0.05                 # STEER_ANGLE_RATE
    coeffs[10] = 1e-7                # WHEEL_FORCE_UP_MAX
    coeffs[12] = 1e-7                # WHEEL_FORCE_SIDE_MAX
    coeffs[17] = coeffs[18] = 5.0    # UNCERTAINTY_POS_X / _Y
    cost.s_coeffs[:] = coeffs
    cost.s_goal[:] = goal
    dyn = m.RacerDubinsSuspensionParams()
    b = dyn.base
    b.c_0 = 0.0
    b.c_t[:] = [5.0, 5.0, 5.0]
    b.c_v[:] = [1.0, 1.0, 1.0]
    b.c_b[:] = [20.0, 20.0, 20.0]
    b.wheel_base = 2.981
    b.steer_angle_scale = -2.45
    x0 = np.zeros(NS_SUSPENSION, np.float32)
    x0[:8] = [1.0, 0.2, -4.0, -2.0, 0.03, 0.0, 0.0, 0.0]
    x0[13:17] = [0.01, 0.01, 0.001, 0.02]
    blobs = {}
    if maps in ("both", "elevation"):
        z, transform = hills()
        blobs["elevation_map"] = z
        blobs["elevation_map_transform"] = transform
        if maps == "both":
            blobs["normals_map"] = normals_of(z, 0.25)
        # the centre of gravity starts one wheel radius above the terrain under the car
        col, row = int((x0[S_X] + 1.49 + 30.0) / 0.25), int((x0[S_Y] + 30.0) / 0.25)
        x0[S_CGZ] = z[row, col] + 0.32
    else:
        x0[S_CGZ] = 0.32
    blobs.update(steering_blobs(zero=zero_net))
    return dict(model="racer_dubins_elevation_suspension", K=K, T=T, D=D, dt=0.02, lambda_=lambda_, alpha=0.0, num_iters=1,
                dyn=dyn, cost=cost, ranges=[-1.0, 1.0, -1.0, 1.0], std_dev=[0.4, 0.5], control_cost_coeff=[0.0, 0.0], x0=x0,
                blobs=blobs)


def suspension_f64(p, x, height_of, normal_of):
    """float64 restatement of computeSimpleSuspensionStep (…suspension_lstm.cu:199-340): (acc_z, acc_roll, acc_pitch, up_max,
    fwd_max, side_max)"""
    roll, pitch, yaw = float(x[S_ROLL]), float(x[S_PITCH]), float(x[S_YAW])
    cr, sr, cp, sp_, cy, sy = math.cos(roll), math.sin(roll), math.cos(pitch), math.sin(pitch), math.cos(yaw), math.sin(yaw)
    M = np.array([[cp * cy, sr * sp_ * cy - cr * sy, cr * sp_ * cy + sr * sy],
                  [cp * sy, sr * sp_ * sy + cr * cy, cr * sp_ * sy - sr * cy],
                  [-sp_, sr * cp, cr * cp]])
    az = aroll = apitch = 0.0
    up, fwd, side = [], [], []
    for i, (bx, by) in enumerate(WHEELS):
        wyaw = yaw + (4 / -9.1 if i < 2 else 0.0)
        c, s = math.cos(wyaw), math.sin(wyaw)
        world = M @ np.array([bx, by, 0.0]) + np.array([float(x[S_X]), float(x[S_Y]), 0.0])
        h = height_of(world)
        n = normal_of(world)
        cgx, cgy = bx - p.c_g[0], by - p.c_g[1]
        pos_z = float(x[S_CGZ]) + roll * cgy - pitch * cgx - p.wheel_radius
        vel_z = float(x[S_CGVZ]) + float(x[S_ROLL_RATE]) * cgy - float(x[S_PITCH_RATE]) * cgx
        h_dot = -(float(x[S_VEL]) * c * n[0] + float(x[S_VEL]) * s * n[1])
        f = -p.spring_k * (pos_z - h) - p.drag_c * (vel_z - h_dot)
        up.append(f)
        fwd.append(abs(f / n[2] * (n[0] * c + n[1] * s + n[2] * -pitch)))
        side.append(abs(f / n[2] * (-n[0] * s + n[1] * c + n[2] * roll)))
        az += f / p.mass
        aroll += f * cgy / p.I_xx
        apitch += -f * cgx / p.I_yy
    return az, aroll, apitch, max(up), max(fwd), max(side)


def st26(*v):
    x = np.zeros(NS_UNCERTAINTY, np.float32)
    x[:len(v)] = v
    return x


def network_blobs(seed=33, scale=0.06, zero=False):
    rng = np.random.default_rng(seed)
    mk = (lambda n: np.zeros(n, np.float32)) if zero else (lambda n: rng.uniform(-scale, scale, n).astype(np.float32))
    return {"mean_lstm_weights": mk(MEAN_LSTM), "mean_lstm_output_weights": mk(MEAN_OUT), "unc_lstm_weights": mk(UNC_LSTM),
            "unc_lstm_output_weights": mk(UNC_OUT)}


def uncertainty_cfg(zero=False, **kw):
    cfg = suspension_cfg(zero_net=zero, **kw)
    cfg["model"] = "racer_dubins_elevation_lstm_unc"
    dyn = m.RacerDubinsUncertaintyParams()
    src = cfg["dyn"]
    C_bytes = bytes(src)
    import ctypes as C
    C.memmove(C.addressof(dyn.suspension), C_bytes, len(C_bytes))
    dyn.unc_scale[:] = [1e-3] * 7   # the networks are random: keep their process noise from dominating the cost
    cfg["dyn"] = dyn
    x0 = np.zeros(NS_UNCERTAINTY, np.float32)
    x0[:13] = cfg["x0"][:13]
    x0[UNC:UNC + 4] = [0.01, 0.01, 0.001, 0.02]
    cfg["x0"] = x0
    cfg["blobs"].update(network_blobs(zero=zero))
    return cfg
