"""RacerDubinsElevation + QuadraticCost: the RACER Dubins car on an elevation map with a propagated
4x4 covariance (reference: dynamics/racer_dubins/racer_dubins_elevation.cu, racer_dubins.cu:358-434 static settling).

Pinning.  The reference's own known answers for this model are tests/dynamics/racer_dubins_elevation_model_test.cu TestStep
(:305-605) and TestStepReverse (:694-913); ComputeDynamics / TestUpdateState there are commented out.  Those answers are the
HOST flavour; on the tested inputs it differs from the device flavour restated by the oracle only in the math library
(angles are inside (-pi, pi], the covariance states are not looked at).  Some entries of that file no longer follow from
the reference's own source at this snapshot: they encode an earlier revision in which the lowest speed regime reached up
to 0.55 m/s (and scaled with dt) and the brake state was not capped at 0.25 (racer_dubins_elevation.cu:37-52 now reads
linear_brake_slope = 0.2 and fmin(fmax(brake, 0), 0.25)).  Entries marked STALE below are therefore checked against the
value the reference's SOURCE gives (derivation in the comment), not against the number in the test file; every other entry
is checked against the reference's number at the reference's tolerance."""
import math

import numpy as np
import pytest

import pyoracle as po
from common import host_noise, m, make_engine, make_oracle, ulp_diff
from racer_cfgs import elevation_cfg, st  # bench.py imports elevation_cfg from this module

YAW = math.pi / 6
STEER = math.pi / 8
PITCH = 20 * math.pi / 180
S_VEL, S_YAW, S_X, S_Y, S_STEER, S_BRAKE, S_ROLL, S_PITCH, S_STEER_RATE = range(9)
O_POS_Z, O_ACCEL_X = 4, 13


def test_step_params(gear_sign=1):
    """parameters of TestStep (:312-327)"""
    p = m.RacerDubinsElevationParams()
    b = p.base
    b.c_0 = 0
    b.c_b[:] = [1, 10, 100]
    b.c_v[:] = [0.25, 0.5, 0.75]
    b.c_t[:] = [2, 20, 200]
    b.low_min_throttle = 0.2
    b.steer_command_angle_scale = 0.5
    b.steering_constant = 0.5
    b.wheel_base = 0.5
    b.max_steer_rate = 5
    b.gear_sign = gear_sign
    return p


test_step_params.__test__ = False


G = 9.81
YAW_RATE = -0.086361105  # (1 / 0.5) * tan((pi / 8) / -9.1)
STEER_RATE = (0.25 - STEER) * 0.5
# (state, control, dt, expected acceleration, expected next state[0..8], stale?)  — TestStep :336-604 in order
STEP_KAT = [
    (st(), [0, 0], 0.1, 0.0, [0, 0, 0, 0, 0, 0, 0, 0, 0], False),
    # STALE: the file expects -0.115 (regime 0).  Source: |0.54| > 0.2 -> regime 1: 20 * 0.21 - 0.5 * 0.54 = 3.93
    (st(0.54), [0.21, 0], 0.1, 3.93, [0.54 + 0.393, 0, 0.054, 0, 0, 0, 0, 0, 0], True),
    (st(0.56), [0.01, 0], 0.1, -0.08, [0.552, 0, 0.056, 0, 0, 0, 0, 0, 0], False),
    # STALE: the file expects -0.12 (regime 0 because of dt = 0.2).  Source: regime 1: 20 * 0.21 - 0.5 * 0.56 = 3.92
    (st(0.56), [0.21, 0], 0.2, 3.92, [0.56 + 0.784, 0, 0.112, 0, 0, 0, 0, 0, 0], True),
    (st(2.99), [0.01, 0], 0.1, -1.295, [2.8605, 0, 0.299, 0, 0, 0, 0, 0, 0], False),
    (st(3.01), [0.01, 0], 0.1, -0.2575, [2.98425, 0, 0.301, 0, 0, 0, 0, 0, 0], False),
    (st(), [1, 0], 0.1, 1.6, [0.16, 0, 0, 0, 0, 0, 0, 0, 0], False),
    (st(1), [1, 0], 0.1, 5.5, [1.55, 0, 0.1, 0, 0, 0, 0, 0, 0], False),
    (st(), [1, 0.5], 0.1, 1.6, [0.16, 0, 0, 0, 0.5 ** 3 * 0.1, 0, 0, 0, 0.5 ** 3], False),
    (st(1.0, YAW), [1, 0.5], 0.1, 5.5, [1.55, YAW, math.cos(YAW) * 0.1, math.sin(YAW) * 0.1, 0.5 ** 3 * 0.1, 0, 0, 0, 0.5 ** 3], False),
    (st(1.0, YAW, 0, 0, STEER), [1, 0.5], 0.1, 5.5,
     [1.55, YAW + YAW_RATE * 0.1, math.cos(YAW) * 0.1, math.sin(YAW) * 0.1, STEER + STEER_RATE * 0.1, 0, 0, 0, STEER_RATE], False),
    # STALE from here on in the acceleration only: the file expects the brake state 1.0 to act in full (-10 - 0.5 -> clamp
    # -5.5); the source caps it at 0.25: 10 * 0.25 * -1 - 0.5 * 1 = -3.0 (and +2.5 + 0.5 = +3.0 when rolling backwards)
    (st(1.0, YAW, 0, 0, STEER, 1.0), [-1, 0.5], 0.1, -3.0,
     [1 - 0.3, YAW + YAW_RATE * 0.1, math.cos(YAW) * 0.1, math.sin(YAW) * 0.1, STEER + STEER_RATE * 0.1, 1.0, 0, 0, STEER_RATE], True),
    (st(1.0, YAW, 0, 0, STEER, 1.0, 0, PITCH), [-1, 0.5], 0.1, -3.0 + G * math.sin(PITCH),
     [1 + (-3.0 + G * math.sin(PITCH)) * 0.1, YAW + YAW_RATE * 0.1, math.cos(YAW) * 0.1, math.sin(YAW) * 0.1,
      STEER + STEER_RATE * 0.1, 1.0, 0, 0, STEER_RATE], True),
    (st(-1.0, YAW, 0, 0, STEER, 1.0, 0, PITCH), [-1, 0.5], 0.1, 3.0 + G * math.sin(PITCH),
     [-1 + (3.0 + G * math.sin(PITCH)) * 0.1, YAW - YAW_RATE * 0.1, -math.cos(YAW) * 0.1, -math.sin(YAW) * 0.1,
      STEER + STEER_RATE * 0.1, 1.0, 0, 0, STEER_RATE], True),
    (st(-1.0, YAW, 0, 0, STEER, 1.0, 0, PITCH), [-1, -0.5], 0.1, 3.0 + G * math.sin(PITCH),
     [-1 + (3.0 + G * math.sin(PITCH)) * 0.1, YAW - YAW_RATE * 0.1, -math.cos(YAW) * 0.1, -math.sin(YAW) * 0.1,
      STEER + (-0.25 - STEER) * 0.5 * 0.1, 1.0, 0, 0, (-0.25 - STEER) * 0.5], True),
    (st(-1.0, YAW, 0, 0, STEER * 100, 1.0, 0, PITCH), [-1, -0.5], 0.1, 3.0 + G * math.sin(PITCH),
     [-1 + (3.0 + G * math.sin(PITCH)) * 0.1, YAW + math.tan(STEER * 100 / -9.1) * 0.1 * -2, -math.cos(YAW) * 0.1,
      -math.sin(YAW) * 0.1, 0.5, 1.0, 0, 0, -5.0], True),
]


def test_oracle_reproduces_reference_test_step():
    """reference tolerance 1e-6 (absolute); 4e-6 on the two entries whose value passes through tan() of a large angle or
    sits at 2.98 (the det_math.h functions and one fp32 rounding differ from the host's libm in the last bits)"""
    o = po.Oracle("racer_dubins_elevation", 64, 4, 1, 0.1, 1.0, 0.0, 1)
    o.set_dynamics_params(test_step_params())
    n_live = 0
    for x, u, dt, acc, want, stale in STEP_KAT:
        xn, xd, y = o.model_step_full(x, np.array(u, np.float32), dt)
        tol = 4e-6
        assert abs(xd[S_VEL] - acc) <= tol, (x[:8], u, xd[S_VEL], acc)
        assert abs(y[O_ACCEL_X] - acc) <= tol
        for i in range(9):
            assert abs(xn[i] - want[i]) <= tol, (x[:8], u, i, xn[i], want[i])
        n_live += not stale
    assert n_live == 9


def test_oracle_reproduces_reference_test_step_reverse():
    """TestStepReverse (:694-913): gear_sign = -1 turns the throttle around (full throttle from rest: -1.6, :741-754; at
    v = 1: -20 - 0.5 -> clamp -5.5, :756-770); the braking entries (:860-912) are those of TestStep"""
    o = po.Oracle("racer_dubins_elevation", 64, 4, 1, 0.1, 1.0, 0.0, 1)
    o.set_dynamics_params(test_step_params(gear_sign=-1))
    xn, xd, y = o.model_step_full(st(), np.array([1, 0], np.float32), 0.1)
    assert abs(xd[S_VEL] + 1.6) <= 1e-6 and abs(xn[S_VEL] + 0.16) <= 1e-6 and abs(y[O_ACCEL_X] + 1.6) <= 1e-6
    xn, xd, y = o.model_step_full(st(1), np.array([1, 0], np.float32), 0.1)
    assert abs(xd[S_VEL] + 5.5) <= 1e-6 and abs(xn[S_VEL] - 0.45) <= 1e-6 and abs(xn[S_X] - 0.1) <= 1e-6
    xn, xd, y = o.model_step_full(st(-1.0, YAW, 0, 0, STEER, 1.0, 0, PITCH), np.array([-1, 0.5], np.float32), 0.1)
    assert abs(xd[S_YAW] + YAW_RATE) <= 1e-6 and abs(xn[S_STEER_RATE] - STEER_RATE) <= 1e-6
    assert abs(xd[S_VEL] - (3.0 + G * math.sin(PITCH))) <= 4e-6


def covariance_step_f64(p, x, xdot, dt):
    """float64 restatement of computeUncertaintyJacobian / computeQ / computeUncertaintyPropagation (device flavour)"""
    b = p.base
    v, yaw, steer, brake, roll = float(x[S_VEL]), float(x[S_YAW]), float(x[S_STEER]), float(x[S_BRAKE]), float(x[S_ROLL])
    idx = (0.2 < abs(v) <= 3.0) + 2 * (abs(v) > 3.0)
    bs = min(max(brake, 0.0), 0.25)
    delta = steer / b.steer_angle_scale
    s, c, t, c2 = math.sin(yaw), math.cos(yaw), math.tan(delta), math.cos(delta) ** 2
    A = np.zeros((4, 4))
    A[0] = [-b.c_v[idx] - p.K_vel_x - (idx == 0) * b.c_b[0] * bs, 0, -p.K_x * c, -p.K_x * s]
    A[1] = [t / b.wheel_base, -abs(v) * p.K_yaw / (b.wheel_base * c2), v * p.K_y * s / (b.wheel_base * c2),
            -v * p.K_y * c / (b.wheel_base * c2)]
    A[2] = [c, -s * v, 0, 0]
    A[3] = [s, c * v, 0, 0]
    side = v * v * t / b.wheel_base + b.gravity * math.sin(roll)
    q11 = abs(p.Q_y_f * abs(side) * max(abs(v) - 2, 0.0))
    Q = np.zeros((4, 4))
    Q[0, 0] = p.Q_x_acc * abs(float(xdot[S_VEL])) + p.Q_x_v[idx] * abs(v)
    Q[1, 1] = abs(v) * (p.Q_omega_steering * abs(delta) + p.Q_omega_v)
    Q[2, 2], Q[3, 3], Q[2, 3] = q11 * s * s, q11 * c * c, -q11 * s * c
    Q[3, 2] = Q[2, 3]
    # state order: POS_X, POS_Y, YAW, VEL_X, POS_X_Y, POS_X_YAW, POS_X_VEL_X, POS_Y_YAW, POS_Y_VEL_X, YAW_VEL_X (9..18);
    # matrix order (v, yaw, x, y)
    u = [float(t_) for t_ in x[9:19]]
    S = np.array([[u[3], u[9], u[6], u[8]], [u[9], u[2], u[5], u[7]], [u[6], u[5], u[0], u[4]], [u[8], u[7], u[4], u[1]]])
    F = np.eye(4) + A * dt
    Sn = F @ S @ F.T + Q * dt
    return np.array([Sn[2, 2], Sn[3, 3], Sn[1, 1], Sn[0, 0], Sn[3, 2], Sn[2, 1], Sn[2, 0], Sn[3, 1], Sn[3, 0], Sn[1, 0]])


def test_oracle_covariance_propagation_against_float64():
    rng = np.random.default_rng(5)
    p = m.RacerDubinsElevationParams()
    p.Q_omega_steering = 0.02
    o = po.Oracle("racer_dubins_elevation", 64, 4, 1, 0.02, 1.0, 0.0, 1)
    o.set_dynamics_params(p)
    for trial in range(200):
        x = st(rng.uniform(-6, 6), rng.uniform(-3, 3), rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(-0.5, 0.5),
               rng.uniform(0, 1), rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), 0.0)
        L = rng.uniform(-0.3, 0.3, (4, 4))
        S = L @ L.T  # (v, yaw, x, y)
        x[9:19] = [S[2, 2], S[3, 3], S[1, 1], S[0, 0], S[3, 2], S[2, 1], S[2, 0], S[3, 1], S[3, 0], S[1, 0]]
        u = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1)], np.float32)
        xn, xd, y = o.model_step_full(x, u, 0.02)
        want = covariance_step_f64(p, x, xd, 0.02)
        assert np.abs(xn[9:19] - want).max() <= 2e-5 * max(1.0, np.abs(want).max()), (trial, xn[9:19], want)
        # outputs 17..26 carry the covariance in the state's order
        assert np.array_equal(y[17:27], xn[9:19])
        assert np.isnan(y[10:13]).all() and y[16] == abs(xn[S_VEL]) and y[27] == 0


def plane_map(slope_x, slope_y, n=200, res=0.25, origin=(-25.0, -25.0, 0.0)):
    """heights of the plane z = slope_x * X + slope_y * Y sampled at the cell centres; (blob, transform)"""
    centres = (np.arange(n) + 0.5) * res
    X = origin[0] + centres[None, :]
    Y = origin[1] + centres[:, None]
    heights = (slope_x * X + slope_y * Y).astype(np.float32)
    transform = np.array(list(origin) + [1, 0, 0, 0, 1, 0, 0, 0, 1] + [res, res, 1.0], np.float32)
    return heights, transform


def test_oracle_static_settling_on_a_plane():
    """on a plane the bilinear lookups are exact, so roll / pitch / height follow from the geometry of
    RACER::computeStaticSettling (racer_dubins.cu:358-434): wheel contact points from the CURRENT roll / pitch (here 0),
    pitch = asin(-(h_front - h_rear) / 2.981), roll = asin((h_left - h_right) / 1.474), height = mean of the rear wheels"""
    o = po.Oracle("racer_dubins_elevation", 64, 4, 1, 0.02, 1.0, 0.0, 1)
    sx, sy = 0.08, -0.05
    heights, transform = plane_map(sx, sy)
    o.set_blob("elevation_map", heights)
    o.set_blob("elevation_map_transform", transform)
    for yaw in (0.0, 0.7, -2.1, 3.0):
        x = st(0.0, yaw, 1.5, -2.0)
        xn, xd, y = o.model_step_full(x, np.zeros(2, np.float32), 0.02)
        c, s = math.cos(xn[S_YAW]), math.sin(xn[S_YAW])
        px, py = float(xn[S_X]), float(xn[S_Y])

        def h(bx, by):
            return sx * (px + c * bx - s * by) + sy * (py + s * bx + c * by)

        fl, fr, rl, rr = h(2.981, 0.737), h(2.981, -0.737), h(0, 0.737), h(0, -0.737)
        roll = (math.asin((fl - fr) / 1.474) + math.asin((rl - rr) / 1.474)) / 2
        pitch = (math.asin((rl - fl) / 2.981) + math.asin((rr - fr) / 2.981)) / 2
        assert abs(xn[S_ROLL] - roll) <= 2e-5 and abs(xn[S_PITCH] - pitch) <= 2e-5, (yaw, xn[S_ROLL], roll, xn[S_PITCH], pitch)
        assert abs(y[O_POS_Z] - (rl + rr) / 2) <= 2e-5
    # without a map the car settles flat (texture not in use, racer_dubins.cu:426-431)
    o2 = po.Oracle("racer_dubins_elevation", 64, 4, 1, 0.02, 1.0, 0.0, 1)
    xn, xd, y = o2.model_step_full(st(1.0, 0.3, 0, 0, 0, 0, 0.2, 0.1), np.zeros(2, np.float32), 0.02)
    assert xn[S_ROLL] == 0 and xn[S_PITCH] == 0 and y[O_POS_Z] == 0
    # a cliff: the height differences are clamped before asin (0.736 * 2 over the track, 2.98 along the wheel base)
    cliff = np.zeros((200, 200), np.float32)
    cliff[:, 104:] = 50.0
    o.set_blob("elevation_map", cliff)
    xn, xd, y = o.model_step_full(st(0.0, 0.0, 0.0, 0.0), np.zeros(2, np.float32), 0.02)
    assert abs(xn[S_PITCH] + math.asin(2.98 / 2.981)) <= 1e-4 and np.isfinite(xn).all()


def test_oracle_closed_loop_over_the_hills():
    cfg = elevation_cfg(K=512, T=40)
    o = make_oracle(cfg)
    x = cfg["x0"].copy()
    rolls = []
    for i in range(60):
        o.vanilla_compute_control(x, 1, host_noise(1, cfg["K"], cfg["T"], 2, seed=100 + i))
        u = o.control()[0].copy()
        x, _ = o.model_step(x, u)
        o.vanilla_slide(1)
        rolls.append(abs(x[S_ROLL]) + abs(x[S_PITCH]))
    assert np.isfinite(x).all() and 2.0 < x[S_VEL] < 3.6 and max(rolls) > 0.01   # moving at speed on uneven ground
    # the covariance moved (the reference's default Q_x_v fit has negative entries, so it need not grow)
    assert np.abs(x[9:19] - cfg["x0"][9:19]).max() > 1e-3


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("variant,with_map", [(1, True), (2, True), (2, False)])
def test_elevation_rollout_costs_bit_exact(gpu, variant, with_map):
    cfg = elevation_cfg(K=1000, T=60, with_map=with_map)
    eps = host_noise(1, cfg["K"], cfg["T"], 2, seed=3)
    o = make_oracle(cfg)
    o.vanilla_compute_control(cfg["x0"], 1, eps)
    eng = make_engine(cfg, kernel_variant=variant)
    eng.injectNoise(eps)
    eng.computeControl(cfg["x0"], 1)
    assert np.isfinite(o.costs()).all()
    assert ulp_diff(eng.getSampledCostSeq(), o.costs()).max() == 0
    assert np.abs(eng.getControlSeq() - o.control()).max() <= 1e-5
    assert np.abs(eng.getTargetStateSeq() - o.state_traj()).max() <= 1e-4
    y = eng.getTargetOutputSeq()
    xs, ys = o.output_trajectory(cfg["x0"], o.control())
    finite = np.isfinite(ys)
    assert np.array_equal(np.isfinite(y), finite) and np.abs(y[finite] - ys[finite]).max() <= 1e-4
    if with_map:
        assert np.abs(ys[:, 6]).max() > 1e-3 and np.abs(ys[:, 4]).max() > 1e-2   # roll and height vary along the trajectory


@pytest.mark.gpu
@pytest.mark.parametrize("variant,with_map,D", [(1, True, 1), (2, True, 1), (2, False, 1), (1, True, 2)])
def test_elevation_four_lanes_per_rollout_bit_exact(gpu, variant, with_map, D):
    """RacerDubinsElevationQuad (block shape (64, 4)): wheels, covariance rows and angles of a step shared out over four
    replica lanes — same bits as the one-lane form and the oracle; fused and role-pipelined kernel, Tube"""
    cfg = elevation_cfg(K=1000, T=60, with_map=with_map, D=D)
    eps = host_noise(1, cfg["K"], cfg["T"], 2, seed=3)
    o = make_oracle(cfg)
    if D == 2:
        o.tube_compute_control(cfg["x0"], 1, eps)
    else:
        o.vanilla_compute_control(cfg["x0"], 1, eps)
    eng = make_engine(cfg, block_x=64, block_y=4, kernel_variant=variant)
    eng.injectNoise(eps)
    eng.computeControl(cfg["x0"], 1)
    assert ulp_diff(eng.getSampledCostSeq(), o.costs()).max() == 0
    assert np.abs(eng.getControlSeq() - o.control()).max() <= 1e-5
    assert np.abs(eng.getTargetStateSeq() - o.state_traj()).max() <= 1e-4
    if D == 1:
        y = eng.getTargetOutputSeq()
        xs, ys = o.output_trajectory(cfg["x0"], o.control())
        finite = np.isfinite(ys)
        assert np.array_equal(np.isfinite(y), finite) and np.abs(y[finite] - ys[finite]).max() <= 1e-4


@pytest.mark.gpu
def test_elevation_model_step_equals_oracle(gpu):
    """modelStep on the device (enforceConstraints + step) against the oracle, bit for bit: the reference's TestStep inputs
    and random states over the map"""
    cfg = elevation_cfg(K=256, T=20)
    cfg["dyn"] = test_step_params()
    cfg["ranges"] = None
    o = make_oracle(cfg)
    eng = make_engine(cfg)
    for x, u, dt, acc, want, stale in STEP_KAT:
        xe, ue = eng.modelStep(x, np.array(u, np.float32), dt=dt)
        xo, uo = o.model_step(x, np.array(u, np.float32), dt=dt)
        assert ulp_diff(xe, xo).max() == 0, (x[:8], u, xe, xo)
    rng = np.random.default_rng(11)
    for trial in range(100):
        x = st(rng.uniform(-6, 6), rng.uniform(-3, 3), rng.uniform(-20, 20), rng.uniform(-20, 20), rng.uniform(-0.5, 0.5),
               rng.uniform(0, 1), rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), 0.0)
        x[9:19] = rng.uniform(-0.05, 0.05, 10)
        u = rng.uniform(-1, 1, 2).astype(np.float32)
        xe, ue = eng.modelStep(x, u)
        xo, uo = o.model_step(x, u)
        same = (xe.view(np.uint32) == xo.view(np.uint32)) | (np.isnan(xe) & np.isnan(xo))
        assert same.all(), (trial, x, u, xe, xo)


@pytest.mark.gpu
def test_elevation_tube_and_closed_loop(gpu):
    cfg = elevation_cfg(K=1024, T=50, D=2)
    eps = host_noise(1, cfg["K"], cfg["T"], 2, seed=4)
    o = make_oracle(cfg)
    o.tube_compute_control(cfg["x0"], 1, eps)
    eng = make_engine(cfg)
    eng.injectNoise(eps)
    eng.computeControl(cfg["x0"], 1)
    assert ulp_diff(eng.getSampledCostSeq(), o.costs()).max() == 0
    assert np.abs(eng.getControlSeq() - o.control()).max() <= 1e-5
    # closed loop on the device's own noise
    cfg = elevation_cfg(K=2048, T=50)
    eng = make_engine(cfg)
    x = cfg["x0"].copy()
    for i in range(80):
        eng.computeControl(x, 1)
        u = eng.getControlSeq()[0].copy()
        x, _ = eng.modelStep(x, u)
        eng.slideControlSequence(1)
    assert np.isfinite(x).all() and 2.0 < x[S_VEL] < 3.6


@pytest.mark.gpu
def test_elevation_colored_noise_runs(gpu):
    """ColoredMPPI over the elevation model (the sampler of the reference's RACER controllers): finite, and it drives"""
    cfg = elevation_cfg(K=1024, T=64)
    cfg["colored"] = ([1.0, 1.0], 0.97, 0.0)
    eng = make_engine(cfg)
    x = cfg["x0"].copy()
    for i in range(60):
        eng.computeControl(x, 1)
        u = eng.getControlSeq()[0].copy()
        x, _ = eng.modelStep(x, u)
        eng.slideControlSequence(1)
    assert np.isfinite(x).all() and np.isfinite(eng.getControlSeq()).all() and x[S_VEL] > 1.5


def test_oracle_racer_leash_in_body_frame():
    """RacerDubinsImpl::enforceLeash (racer_dubins.cu:176-240) through ColoredMPPI's leash: a position error of (3, 0) in the
    map frame for a car heading 90 deg left is (0, -3) in its body frame, so the y leash limits it; yaw takes the short way
    round"""
    cfg = elevation_cfg(K=64, T=8, with_map=False)
    o = make_oracle(cfg)
    leash = np.full(19, 100.0, np.float32)
    leash[S_X], leash[S_Y], leash[S_YAW] = 1.0, 0.5, 0.2
    o.set_colored_mppi_params(0.0, 0.0, leash, True, 1)
    # nominal trajectory: put a known state at index 1 through one compute_control from a chosen start
    x_true = st(0.0, math.pi / 2, 0.0, 0.0)
    nominal = st(0.0, -math.pi + 0.1, 3.0, 0.0)
    out = o.enforce_leash(x_true, nominal, leash)
    # body frame of the true state (x forward = +Y map): dx_body = dx cos + dy sin = 0, dy_body = -dx sin + dy cos = -3 -> -0.5
    assert abs(out[S_X] - 0.5) <= 1e-6 and abs(out[S_Y]) <= 1e-6
    # yaw: from pi/2 to -pi + 0.1 the short way is +(pi/2 + 0.1) -> limited to +0.2
    assert abs(out[S_YAW] - (math.pi / 2 + 0.2)) <= 1e-6
    assert out[S_VEL] == nominal[S_VEL]


@pytest.mark.gpu
def test_elevation_colored_mppi_leash_parity(gpu):
    """ColoredMPPI with the state leash on the elevation model: the engine applies the RACER body-frame rule on the host
    (has_host_leash) as the oracle does; closed loop with a drifting measured state"""
    cfg = elevation_cfg(K=1024, T=48)
    cfg["colored"] = ([1.0, 1.0], 0.97, 0.0)
    from common import host_spectrum
    eng, orc = make_engine(cfg), make_oracle(cfg)
    leash = np.full(19, 0.5, np.float32)
    leash[S_X], leash[S_Y], leash[S_YAW], leash[S_VEL] = 0.3, 0.1, 0.05, 0.2
    eng.setColoredMPPIParams(gamma=0.0, r_exp=0.0, state_leash_dist=leash, leash_active=True, leash_jump=1)
    orc.set_colored_mppi_params(0.0, 0.0, leash, True, 1)
    exps, decay, fmin = cfg["colored"]
    x = cfg["x0"].copy()
    for i in range(4):
        z = host_spectrum(1, cfg["K"], cfg["T"], 2, seed=60 + i)
        eng.injectNoise(z)
        eng.computeControl(x, 1)
        orc.colored_compute_control(x, 1, z, exps, decay, fmin)
        assert np.abs(eng.getControlSeq() - orc.control()).max() <= 1e-5
        assert np.abs(eng.getTargetStateSeq() - orc.state_traj()).max() <= 1e-4
        x, _ = orc.model_step(x, orc.control()[0])
        x[:4] += np.array([0.3, 0.1, 0.4, -0.3], np.float32)   # the measured state drifts: the leash has something to do
        eng.slideControlSequence(1)
        orc.vanilla_slide(1)
