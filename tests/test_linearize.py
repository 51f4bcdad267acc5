"""computeGrad of the five shipped Dynamics classes, built for the host, against float64 (CPU; the device side is
tests/test_linearize_gpu.py).

The reference per model is this file's own text: the continuous dynamics f(x, u) and its Jacobian in numpy float64 — analytic for
the cartpole, the double integrator and RacerDubins, central differences of f for the quadrotor (f is quadratic in the quaternion
and bilinear in (quaternion, body rates): the differences are exact up to float64 rounding), the chain rule
W3 diag(1 - h2^2) W2 diag(1 - h1^2) W1 for the network.  Every analytic Jacobian is itself held to central differences of f.

Tolerance: the same formula evaluated in numpy float32 deviates from float64 by what the number format costs; the largest such
deviation over the model's test points, any entry, is the yardstick, and the shipped class gets 4 x that per entry (room for
another order of operations, not for another formula).  Measured on this file's points (test_shipped_class_against_float64
prints them):

    model               yardstick (fp32 formula vs fp64)   bound (4 x)    shipped class, largest deviation
    cartpole            5.81e-06                            2.32e-05       8.26e-06
    double_integrator   0                                   0              0
    racer_dubins        4.39e-07                            1.75e-06       2.14e-07
    quadrotor           3.77e-06                            1.51e-05       3.77e-06
    autorally_nn        8.80e-07                            3.52e-06       1.25e-06
"""
import os

import numpy as np
import pytest

import linearize_cases as lc
import linearize_host as lh
import native_build as nb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 9.81


def wrap(a, dt):
    """angle -> (-pi, pi], in the arithmetic of dt (the models wrap before sin / cos)"""
    two_pi = dt(2 * np.pi)
    return dt(a - two_pi * np.round(a / two_pi))


# ---- cartpole -------------------------------------------------------------------------------------------------------------------
def cartpole_f(x, u, p):
    mc, mp, l = (float(v) for v in p)
    s, c, w, F = np.sin(x[2]), np.cos(x[2]), x[3], u[0]
    den = mc + mp * s * s
    return np.array([x[1], (F + mp * s * (l * w * w + G * c)) / den, w,
                     (-F * c - mp * l * w * w * c * s - (mc + mp) * G * s) / (l * den)])


def cartpole_jac(x, u, p, dt):
    mc, mp, l, g = dt(p[0]), dt(p[1]), dt(p[2]), dt(G)
    th = wrap(dt(x[2]), dt)
    s, c, w, F = np.sin(th), np.cos(th), dt(x[3]), dt(u[0])
    den = mc + mp * s * s
    A, B = np.zeros((4, 4), dt), np.zeros((4, 1), dt)
    A[0, 1] = A[2, 3] = 1
    A[1, 2] = (mp * c * (l * w * w + g * c) - g * mp * s * s) / den - dt(2) * mp * c * s * (F + mp * s * (l * w * w + g * c)) / (den * den)
    A[1, 3] = dt(2) * l * mp * w * s / den
    A[3, 2] = (F * s - g * c * (mp + mc) - l * mp * w * w * c * c + l * mp * w * w * s * s) / (l * den) + \
        dt(2) * mp * c * s * (l * mp * c * s * w * w + F * c + g * s * (mp + mc)) / (l * den * den)
    A[3, 3] = -dt(2) * mp * w * c * s / den
    B[1, 0] = dt(1) / den
    B[3, 0] = -c / (l * den)
    return A, B


# ---- double integrator ----------------------------------------------------------------------------------------------------------
def di_f(x, u, p):
    return np.array([x[2], x[3], u[0], u[1]])


def di_jac(x, u, p, dt):
    A, B = np.zeros((4, 4), dt), np.zeros((4, 2), dt)
    A[0, 2] = A[1, 3] = 1
    B[2, 0] = B[3, 1] = 1
    return A, B


# ---- RacerDubins (default parameters of racer_dubins.cuh:67-87) -----------------------------------------------------------------
RD = dict(c_t=1.3, c_b=2.5, c_v=3.7, c_0=4.9, steering_constant=0.6, steer_command_angle_scale=5.0, steer_angle_scale=-9.1,
          max_steer_rate=5.0, brake_delay_constant=6.6, max_brake_rate_neg=0.9, max_brake_rate_pos=0.33, wheel_base=0.3, gear_sign=1)


def racer_branches(x, u):
    """(braking, brake lag inside its limits, steering lag inside its limits, v >= 0)"""
    brake_rate = ((-u[0] if u[0] < 0 else 0.0) - x[5]) * RD["brake_delay_constant"]
    steer_rate = (u[1] * RD["steer_command_angle_scale"] - x[4]) * RD["steering_constant"]
    return (u[0] < 0, -RD["max_brake_rate_neg"] < brake_rate < RD["max_brake_rate_pos"],
            -RD["max_steer_rate"] < steer_rate < RD["max_steer_rate"], x[0] >= 0)


def racer_f(x, u, p):
    v, yaw, steer, brake = x[0], x[1], x[4], x[5]
    braking = u[0] < 0
    d = np.zeros(7)
    d[5] = min(max(((-u[0] if braking else 0.0) - brake) * RD["brake_delay_constant"], -RD["max_brake_rate_neg"]), RD["max_brake_rate_pos"])
    d[0] = (0.0 if braking else RD["c_t"] * u[0] * RD["gear_sign"]) + RD["c_b"] * brake * (-1 if v >= 0 else 1) - RD["c_v"] * v + RD["c_0"]
    d[1] = v / RD["wheel_base"] * np.tan(steer / RD["steer_angle_scale"])
    d[2], d[3] = v * np.cos(yaw), v * np.sin(yaw)
    d[4] = min(max((u[1] * RD["steer_command_angle_scale"] - steer) * RD["steering_constant"], -RD["max_steer_rate"]), RD["max_steer_rate"])
    return d


def racer_jac(x, u, p, dt):
    P = {k: dt(v) for k, v in RD.items()}
    braking, brake_free, steer_free, forward = racer_branches(np.asarray(x, np.float64), np.asarray(u, np.float64))
    v, yaw, steer = dt(x[0]), wrap(dt(x[1]), dt), dt(x[4])
    A, B = np.zeros((7, 7), dt), np.zeros((7, 2), dt)
    if brake_free:
        A[5, 5] = -P["brake_delay_constant"]
        if braking:
            B[5, 0] = -P["brake_delay_constant"]
    A[0, 0] = -P["c_v"]
    A[0, 5] = -P["c_b"] if forward else P["c_b"]
    if not braking:
        B[0, 0] = P["c_t"] * P["gear_sign"]
    t = np.tan(steer / P["steer_angle_scale"])
    A[1, 0] = t / P["wheel_base"]
    A[1, 4] = (v / P["wheel_base"]) * ((dt(1) + t * t) / P["steer_angle_scale"])
    A[2, 0], A[2, 1] = np.cos(yaw), -(v * np.sin(yaw))
    A[3, 0], A[3, 1] = np.sin(yaw), v * np.cos(yaw)
    if steer_free:
        A[4, 4] = -P["steering_constant"]
        B[4, 1] = P["steer_command_angle_scale"] * P["steering_constant"]
    return A, B


# ---- quadrotor ------------------------------------------------------------------------------------------------------------------
def quadrotor_f(x, u, p):
    tau, mass = np.asarray(p[:3], np.float64), float(p[3])
    q, w = x[6:10], x[10:13]
    body_z = np.array([2 * (q[1] * q[3] + q[0] * q[2]), 2 * (q[2] * q[3] - q[0] * q[1]), q[0] ** 2 - q[1] ** 2 - q[2] ** 2 + q[3] ** 2])
    d = np.zeros(13)
    d[0:3] = x[3:6]
    d[3:6] = u[3] / mass * body_z - np.array([0, 0, G])
    d[6] = 0.5 * (-w[0] * q[1] - w[1] * q[2] - w[2] * q[3])
    d[7] = 0.5 * (w[0] * q[0] - w[1] * q[3] + w[2] * q[2])
    d[8] = 0.5 * (w[0] * q[3] + w[1] * q[0] - w[2] * q[1])
    d[9] = 0.5 * (-w[0] * q[2] + w[1] * q[1] + w[2] * q[0])
    d[10:13] = (u[0:3] - w) / tau
    return d


def quadrotor_jac(x, u, p, dt):
    """the analytic form, for the float32 yardstick (the float64 reference is central differences of quadrotor_f)"""
    tau, mass = [dt(v) for v in p[:3]], dt(p[3])
    q, w = [dt(v) for v in x[6:10]], [dt(v) for v in x[10:13]]
    A, B = np.zeros((13, 13), dt), np.zeros((13, 4), dt)
    A[0:3, 3:6] = np.eye(3, dtype=dt)
    acc, two, half = dt(u[3]) / mass, dt(2), dt(0.5)
    dz = [[q[2], q[3], q[0], q[1]], [-q[1], -q[0], q[3], q[2]], [q[0], -q[1], -q[2], q[3]]]
    body_z = [two * (q[1] * q[3] + q[0] * q[2]), two * (q[2] * q[3] - q[0] * q[1]), q[0] * q[0] - q[1] * q[1] - q[2] * q[2] + q[3] * q[3]]
    for i in range(3):
        for j in range(4):
            A[3 + i, 6 + j] = acc * (two * dz[i][j])
        B[3 + i, 3] = body_z[i] / mass
        A[10 + i, 10 + i] = -dt(1) / tau[i]
        B[10 + i, i] = dt(1) / tau[i]
    hw, hq = [half * v for v in w], [half * v for v in q]
    A[6:10, 6:10] = [[0, -hw[0], -hw[1], -hw[2]], [hw[0], 0, hw[2], -hw[1]], [hw[1], -hw[2], 0, hw[0]], [hw[2], hw[1], -hw[0], 0]]
    A[6:10, 10:13] = [[-hq[1], -hq[2], -hq[3]], [hq[0], -hq[3], hq[2]], [hq[3], hq[0], -hq[1]], [-hq[2], hq[1], hq[0]]]
    return A, B


# ---- AutoRally network model ----------------------------------------------------------------------------------------------------
def autorally_f(x, u, mats):
    W1, b1, W2, b2, W3, b3 = (np.asarray(a, np.float64) for a in mats)
    s, c = np.sin(x[2]), np.cos(x[2])
    h2 = np.tanh(W2 @ np.tanh(W1 @ np.concatenate([x[3:], u]) + b1) + b2)
    return np.concatenate([[c * x[4] - s * x[5], s * x[4] + c * x[5], -x[6]], W3 @ h2 + b3])


def autorally_jac(x, u, mats, dt):
    W1, b1, W2, b2, W3, b3 = (np.asarray(a, dt) for a in mats)
    x, u = np.asarray(x, dt), np.asarray(u, dt)
    s, c = np.sin(x[2]), np.cos(x[2])
    h1 = np.tanh(W1 @ np.concatenate([x[3:], u]) + b1)
    h2 = np.tanh(W2 @ h1 + b2)
    J = W3 @ np.diag(dt(1) - h2 * h2) @ W2 @ np.diag(dt(1) - h1 * h1) @ W1
    A, B = np.zeros((7, 7), dt), np.zeros((7, 2), dt)
    A[0, 2], A[0, 4], A[0, 5] = -s * x[4] - c * x[5], c, -s
    A[1, 2], A[1, 4], A[1, 5] = c * x[4] - s * x[5], s, c
    A[2, 6] = -1
    A[3:, 3:] = J[:, :4]
    B[3:, :] = J[:, 4:]
    return A, B


BLOB, MATS = lc.autorally_weights()
MODELS = {
    # name: (f, jac, parameter sets as the restatement takes them, the same as host_grad takes them)
    "cartpole": (cartpole_f, cartpole_jac, lc.CARTPOLE_PARAMS, [dict(params=p) for p in lc.CARTPOLE_PARAMS]),
    "double_integrator": (di_f, di_jac, (None,), [dict()]),
    "racer_dubins": (racer_f, racer_jac, (None,), [dict()]),
    "quadrotor": (quadrotor_f, quadrotor_jac, lc.QUADROTOR_PARAMS, [dict(params=p) for p in lc.QUADROTOR_PARAMS]),
    "autorally_nn": (autorally_f, autorally_jac, (MATS,), [dict(weights=BLOB)]),
}
# entries the formulas set (anything else must come back as the engine cleared it)
WRITTEN = {
    "cartpole": ([(0, 1), (1, 2), (1, 3), (2, 3), (3, 2), (3, 3)], [(1, 0), (3, 0)]),
    "double_integrator": ([(0, 2), (1, 3)], [(2, 0), (3, 1)]),
    "racer_dubins": ([(5, 5), (0, 0), (0, 5), (1, 0), (1, 4), (2, 0), (2, 1), (3, 0), (3, 1), (4, 4)], [(5, 0), (0, 0), (4, 1)]),
    "quadrotor": ([(i, 3 + i) for i in range(3)] + [(3 + i, 6 + j) for i in range(3) for j in range(4)] +
                  [(6 + i, 6 + j) for i in range(4) for j in range(4) if i != j] + [(6 + i, 10 + j) for i in range(4) for j in range(3)] +
                  [(10 + i, 10 + i) for i in range(3)], [(3 + i, 3) for i in range(3)] + [(10 + i, i) for i in range(3)]),
    "autorally_nn": ([(0, 2), (0, 4), (0, 5), (1, 2), (1, 4), (1, 5), (2, 6)] + [(3 + i, 3 + j) for i in range(4) for j in range(4)],
                     [(3 + i, j) for i in range(4) for j in range(2)]),
}


def central_differences(f, x, u, p, h=1e-5):
    x, u = np.asarray(x, np.float64), np.asarray(u, np.float64)
    S, C = x.size, u.size
    A, B = np.zeros((S, S)), np.zeros((S, C))
    for j in range(S):
        e = np.zeros(S)
        e[j] = h
        A[:, j] = (f(x + e, u, p) - f(x - e, u, p)) / (2 * h)
    for j in range(C):
        e = np.zeros(C)
        e[j] = h
        B[:, j] = (f(x, u + e, p) - f(x, u - e, p)) / (2 * h)
    return A, B


def reference64(model, x, u, p):
    f, jac = MODELS[model][:2]
    if model == "quadrotor":
        return central_differences(f, x, u, p, h=1e-3)
    return jac(x, u, p, np.float64)


@pytest.mark.parametrize("model", list(MODELS))
def test_float64_jacobian_is_the_derivative_of_f(model):
    """the test's own analytic Jacobians against central differences of the test's own f (float64 both)"""
    f, jac, psets, _ = MODELS[model]
    xs, us = lc.POINTS[model]()
    worst = 0.0
    for p in psets:
        for x, u in zip(xs.astype(np.float64), us.astype(np.float64)):
            if model == "racer_dubins" and (abs(u[0]) < 1e-4 or abs(x[0]) < 1e-4):
                continue  # a difference across a kink is no derivative
            A, B = jac(x, u, p, np.float64)
            An, Bn = central_differences(f, x, u, p, h=1e-6 if model != "quadrotor" else 1e-3)
            scale = 1.0 + max(np.abs(A).max(), np.abs(B).max())
            worst = max(worst, np.abs(A - An).max() / scale, np.abs(B - Bn).max() / scale)
    assert worst < 1e-6, worst


@pytest.mark.parametrize("model", list(MODELS))
def test_shipped_class_against_float64(model):
    _, jac, psets, host_kw = MODELS[model]
    xs, us = lc.POINTS[model]()
    yardstick = shipped = 0.0
    devs = []
    for p, kw in zip(psets, host_kw):
        A_h, B_h, returned = lh.host_grad(model, xs, us, **kw)
        assert returned  # every shipped class has a complete analytic gradient
        for i, (x, u) in enumerate(zip(xs, us)):
            A64, B64 = reference64(model, x.astype(np.float64), u.astype(np.float64), p)
            A32, B32 = jac(x, u, p, np.float32)
            assert A32.dtype == np.float32 and B32.dtype == np.float32
            yardstick = max(yardstick, np.abs(A32 - A64).max(), np.abs(B32 - B64).max())
            devs.append(max(np.abs(A_h[i] - A64).max(), np.abs(B_h[i] - B64).max()))
    shipped = max(devs)
    print("%s: yardstick %.3g, bound %.3g, shipped class %.3g" % (model, yardstick, 4 * yardstick, shipped))
    assert shipped <= 4 * yardstick, (shipped, yardstick)


@pytest.mark.parametrize("model", list(MODELS))
def test_entries_the_formula_does_not_set_are_exactly_zero(model):
    xs, us = lc.POINTS[model]()
    A, B, _ = lh.host_grad(model, xs, us, **MODELS[model][3][-1])
    mask_a, mask_b = np.ones(A.shape[1:], bool), np.ones(B.shape[1:], bool)
    for i, j in WRITTEN[model][0]:
        mask_a[i, j] = False
    for i, j in WRITTEN[model][1]:
        mask_b[i, j] = False
    assert mask_a.sum() > 0 and mask_b.sum() > 0
    assert (A[:, mask_a].view(np.uint32) == 0).all() and (B[:, mask_b].view(np.uint32) == 0).all()  # +0.0f, bit for bit
    # and the written ones are in use: none of them is zero at every point
    assert all(np.any(A[:, i, j] != 0) for i, j in WRITTEN[model][0]) and all(np.any(B[:, i, j] != 0) for i, j in WRITTEN[model][1])


def test_points_reach_every_branch():
    xs, us = lc.racer_dubins_points()
    seen = {racer_branches(x.astype(np.float64), u.astype(np.float64)) for x, u in zip(xs, us)}
    for k in range(4):
        assert {b[k] for b in seen} == {True, False}, k
    th = lc.cartpole_points()[0][:, 2].astype(np.float64)
    for target in (0.0, np.pi / 2, -np.pi / 2, np.pi):
        assert np.abs(th - target).min() < 2e-3
    q = lc.quadrotor_points()[0][:, 6:10].astype(np.float64)
    assert (np.abs(np.linalg.norm(q[1:], axis=1) - 1) > 1e-2).all() and (np.abs(q[1:]) > 1e-3).all()
    # network: units in the linear region and saturated ones
    W1, b1 = MATS[0].astype(np.float64), MATS[1].astype(np.float64)
    xs, us = lc.autorally_points()
    h1 = np.tanh(np.concatenate([xs[:, 3:], us], axis=1).astype(np.float64) @ W1.T + b1)
    assert (np.abs(h1) > 0.999).any() and (np.abs(h1[:12]) < 0.7).all()


def test_double_integrator_matrices_are_the_reference_s():
    """di_dynamics.cu:24-34: A has two ones, B has two ones, whatever the point"""
    xs, us = lc.double_integrator_points()
    A, B, _ = lh.host_grad("double_integrator", xs, us)
    A0, B0 = np.zeros((4, 4), np.float32), np.zeros((4, 2), np.float32)
    A0[0, 2] = A0[1, 3] = B0[2, 0] = B0[3, 1] = 1
    assert (A == A0).all() and (B == B0).all()


def test_network_of_ones_at_the_origin():
    """the configuration of the reference's ARNeuralNetDynamics.computeGrad case (tests/dynamics/ar_dynamics_nn_test.cu:421-442:
    all 1412 parameters one, state and control zero; the case holds no literal values).  The kinematic rows are those of yaw = 0,
    exactly.  Every unit of the second layer sits at tanh(32 tanh(1) + 1), where the true slope 1 - h^2 is 4e-22: the network block
    is zero as far as float32 goes.  det::tanh is within 4e-7 of tanh there (det_math.h), so the slope the class sees is within
    2 * 4e-7 of zero, and each of the 24 entries — 32 * 32 paths of unit weights times that slope times 1 - tanh(1)^2 — within
    32 * 32 * 8e-7 * 0.42 = 3.5e-4; all 24 are the same sum."""
    A, B, _ = lh.host_grad("autorally_nn", np.zeros((1, 7)), np.zeros((1, 2)), weights=np.ones(1412, np.float32))
    A0 = np.zeros((7, 7), np.float32)
    A0[0, 4] = A0[1, 5] = 1
    A0[2, 6] = -1
    assert (A[0, :3] == A0[:3]).all() and (A[0, :, :3] == 0).all() and (B[0, :3] == 0).all()
    block = np.concatenate([A[0, 3:, 3:], B[0, 3:]], axis=1)
    bound = 32 * 32 * 2 * 4e-7 * (1 - np.tanh(1.0) ** 2)
    print("network block of the all-ones case: %.3g (bound %.3g)" % (np.abs(block).max(), bound))
    assert np.abs(block).max() <= bound and (block == block[0, 0]).all()


def test_classes_without_the_method_report_unsupported():
    t = lh.traits()
    for name in ("CartpoleDynamics", "DoubleIntegratorDynamics", "RacerDubins", "QuadrotorDynamics"):
        assert t[name] == (True, False), name
    for name in ("NeuralNetModel", "NeuralNetModelMFMA", "NeuralNetModelWave"):
        assert t[name] == (True, True), name
    for name in ("RacerDubinsElevation", "BicycleSlipLSTM"):
        assert t[name] == (False, False), name


def test_reference_style_example_still_compiles():
    """a plugin written for the reference (no computeGrad in the device form) compiles as before and carries no gradient"""
    probe = os.path.join(REPO, "examples", "_build", "compute_grad_trait_probe.hip")
    os.makedirs(os.path.dirname(probe), exist_ok=True)
    with open(probe, "w") as f:
        f.write('#include "my_model/pendulum_model_reference_style.hip"\n'
                'static_assert(!mppi::has_compute_grad<RefPendulumDynamics>::value, "");\n')
    r = nb.hip_syntax_only(probe, "-I" + os.path.join(REPO, "examples"))
    assert r.returncode == 0, r.stderr[-3000:]


def test_templated_controller_accessor_compiles():
    """controllers_templated.hpp: computeGrad(state, control, A, B) in the reference's spelling and computeGradTrajectory, on the
    cartpole instantiation of the reference's own example (both compiler passes, no code generation)"""
    probe = os.path.join(REPO, "examples", "_build", "compute_grad_templated_probe.hip")
    os.makedirs(os.path.dirname(probe), exist_ok=True)
    with open(probe, "w") as f:
        f.write('#include <mppi/instantiations/cartpole_mppi/cartpole_mppi.cuh>\n#include <vector>\n'
                'using Sampler = mppi::sampling_distributions::GaussianDistribution<CartpoleDynamics::DYN_PARAMS_T>;\n'
                'using Feedback = DDPFeedback<CartpoleDynamics, 100>;\n'
                'using CartpoleMPPI = VanillaMPPIController<CartpoleDynamics, CartpoleQuadraticCost, Feedback, 100, 2048>;\n'
                'bool probe(CartpoleMPPI& c, std::vector<float>& A, std::vector<float>& B)\n{\n'
                '  CartpoleMPPI::state_array x = CartpoleMPPI::state_array::Zero();\n'
                '  CartpoleMPPI::control_array u = CartpoleMPPI::control_array::Zero();\n'
                '  float a[16], b[4];\n  c.computeGradTrajectory(A, B);\n  return c.computeGrad(x, u, a, b);\n}\n')
    r = nb.hip_syntax_only(probe)
    assert r.returncode == 0, r.stderr[-3000:]
