"""Evaluation points of the computeGrad tests (tests/test_linearize.py on the host, tests/test_linearize_gpu.py on the device):
per model a fixed list of (x, u) pairs that reaches every branch of its Jacobian, the parameters they are evaluated with, and
the network weights of the AutoRally model."""
import itertools

import numpy as np

PI = np.pi
CARTPOLE_PARAMS = (np.array([1.0, 1.0, 1.0], np.float32), np.array([1.5, 0.3, 0.7], np.float32))
QUADROTOR_PARAMS = (np.array([0.25, 0.25, 0.25, 1.0], np.float32), np.array([0.2, 0.3, 0.4, 1.7], np.float32))


def cartpole_points():
    """theta at 0, near 0, around +-pi/2 and +-pi, the pi/4 points where d theta_dd / d theta cancels, one past a full turn; with
    theta_dot and force of either sign and zero"""
    thetas = [0.0, 1e-3, -1e-3, PI / 2, -PI / 2, PI / 2 + 0.01, -PI / 2 - 0.01, PI, -PI, PI - 0.01, PI / 4, -3 * PI / 4, 2.5, 7.0]
    pts = [(0.3, -0.4, th, w, f) for th, w, f in itertools.product(thetas, [-3.0, 0.0, 0.5, 2.0], [-8.0, 0.0, 5.0])]
    a = np.array(pts, np.float32)
    return a[:, :4].copy(), a[:, 4:].copy()


def double_integrator_points():
    rng = np.random.default_rng(5)
    return rng.normal(0, 2, (9, 4)).astype(np.float32), rng.normal(0, 2, (9, 2)).astype(np.float32)


def racer_dubins_points():
    """both signs of speed; throttle and brake commands; brake and steering lags inside and on either rate limit; a yaw past pi.
    State [VEL_X, YAW, POS_X, POS_Y, STEER_ANGLE, BRAKE_STATE, STEER_ANGLE_RATE], control [THROTTLE_BRAKE, STEER_CMD]."""
    xs, us = [], []
    for v, yaw, steer, brake, u_tb, u_st in itertools.product([-2.0, 0.5, 3.0], [-2.0, 0.3, 4.0], [-0.4, 0.2], [0.0, 0.3],
                                                             [-0.5, -0.01, 0.4], [-2.0, 0.05, 2.0]):
        xs.append([v, yaw, 1.5, -0.7, steer, brake, 0.1])
        us.append([u_tb, u_st])
    return np.array(xs, np.float32), np.array(us, np.float32)


def quadrotor_points():
    """quaternions that are neither unit nor axis-aligned, every other state and control at ordinary magnitudes, plus level
    hover"""
    rng = np.random.default_rng(11)
    n = 40
    x = rng.normal(0, 1.5, (n, 13)).astype(np.float32)
    x[:, 6:10] = rng.normal(0, 1, (n, 4)) * rng.uniform(0.3, 2.0, (n, 1))
    u = rng.normal(0, 2, (n, 4)).astype(np.float32)
    u[:, 3] = rng.uniform(0, 20, n)
    x[0] = 0
    x[0, 6] = 1
    u[0] = [0, 0, 0, 9.81]
    return x, u


def autorally_weights(scale=0.6, seed=3):
    """a 6-32-32-4 network in the blob order [W1 | b1 | W2 | b2 | W3 | b3] (row-major weights), and its matrices"""
    rng = np.random.default_rng(seed)
    layers = [6, 32, 32, 4]
    mats, blob = [], []
    for i in range(3):
        W = rng.uniform(-scale, scale, (layers[i + 1], layers[i])).astype(np.float32)
        b = rng.uniform(-scale, scale, layers[i + 1]).astype(np.float32)
        mats += [W, b]
        blob += [W.reshape(-1), b]
    return np.concatenate(blob), mats


def autorally_points():
    """inputs small enough for every unit to sit in tanh's linear region, ordinary ones, and large ones that saturate most units.
    State [x, y, yaw, roll, vx, vy, yaw_rate], control [steering, throttle]."""
    rng = np.random.default_rng(17)
    xs, us = [], []
    for mag in (0.02, 1.0, 8.0):
        x = rng.normal(0, 1, (12, 7))
        x[:, 3:] *= mag
        xs.append(x)
        us.append(rng.normal(0, 1, (12, 2)) * mag)
    return np.concatenate(xs).astype(np.float32), np.concatenate(us).astype(np.float32)


POINTS = {"cartpole": cartpole_points, "double_integrator": double_integrator_points, "racer_dubins": racer_dubins_points,
          "quadrotor": quadrotor_points, "autorally_nn": autorally_points}
