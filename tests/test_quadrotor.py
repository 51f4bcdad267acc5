"""The quadrotor model (QuadrotorDynamics + QuadrotorQuadraticCost, registered as "quadrotor") and det::atan2.

CPU: det::atan2 against float64, the quaternion helpers, the CPU restatement (tests/quadrotor_oracle) against an independent
float64 numpy restatement of step and cost, the NaN guard, the registration and what mppi_create refuses.
GPU: every registered shape in both kernel families against the CPU restatement (0 ulp costs, u* within 1e-5), Tube MPPI,
the in-kernel Philox noise, mppi_model_step, det::atan2 on the device, and the reference's hover acceptance test
(tests/controllers/vanilla_mppi_test.cu:160-312) with its literal parameters.
"""
import time

import numpy as np
import pytest

import mppi_generic_amd as m
import pyoracle as po
import quadrotor_oracle as qo
from common import PHILOX_SEED, SEED, U_TOL, host_noise, make_engine, ulp_diff
from restate64 import bits

GRAVITY = np.float32(9.81)


@pytest.fixture(scope="module")
def quadrotor(lib):
    """the registration unit is examples/quadrotor_model/quadrotor_model.hip: built on its own and loaded with
    mppi_load_plugin here, at test time, as tests/test_plugin_model.py does with the pendulum (the kernel-matrix files take
    their lists of registrations when they are imported)"""
    return qo.load_model(m)

REL_TOL = 1e-4  # the reference's own rollout tolerance (tests/mppi_core/rollout_kernel_tests.cu:258)


# ------------------------------------------------------------------ float64 restatement (shares nothing with the C++) ---
def quat_mul64(a, b):
    """Hamilton product from the vector form: (a0 b0 - av.bv, a0 bv + b0 av + av x bv)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.concatenate([[a[0] * b[0] - a[1:] @ b[1:]], a[0] * b[1:] + b[0] * a[1:] + np.cross(a[1:], b[1:])])


def rotation64(q):
    """body-to-world rotation matrix as q v q^-1 applied to the three unit vectors"""
    q = np.asarray(q, np.float64)
    q = q / np.linalg.norm(q)
    qc = q * [1, -1, -1, -1]
    return np.stack([quat_mul64(quat_mul64(q, np.concatenate([[0.0], e])), qc)[1:] for e in np.eye(3)], axis=1)


def euler64(q):
    """roll, pitch, yaw of the 3-2-1 sequence from the rotation matrix (not from the quaternion formulas)"""
    R = rotation64(q)
    return np.array([np.arctan2(R[2, 1], R[2, 2]), -np.arcsin(np.clip(R[2, 0], -1, 1)), np.arctan2(R[1, 0], R[0, 0])])


def step64(x, u, dt, tau=(0.25, 0.25, 0.25), mass=1.0):
    x, u = np.asarray(x, np.float64), np.asarray(u, np.float64)
    q, w = x[6:10], x[10:13]
    xdot = np.zeros(13)
    xdot[0:3] = x[3:6]
    xdot[3:6] = u[3] / mass * rotation64(q)[:, 2] * (q @ q) - [0, 0, 9.81]  # the DCM formulas are not normalised: |q|^2 R
    xdot[6:10] = 0.5 * quat_mul64(q, np.concatenate([[0.0], w]))
    xdot[10:13] = (u[0:3] - w) / np.asarray(tau)
    xn = x + xdot * dt
    qn = xn[6:10]
    xn[6:10] = qn / (np.linalg.norm(qn) * np.copysign(1.0, qn[0]))
    return xn, xdot


def cost64(s, p):
    s, g = np.asarray(s, np.float64), np.asarray(p.s_goal[:], np.float64)
    qs, qg = s[6:10], g[6:10]
    q_diff = quat_mul64(qg, qs * [1, -1, -1, -1] / np.linalg.norm(qs))
    q_diff = q_diff / np.linalg.norm(q_diff)
    d2 = (s - g) ** 2
    total = p.x_coeff * d2[0:3].sum() + p.v_coeff * d2[3:6].sum() + p.w_coeff * d2[10:13].sum()
    if p.use_euler:
        total += (np.array([p.roll_coeff, p.pitch_coeff, p.yaw_coeff]) * euler64(q_diff) ** 2).sum()
    else:
        total += p.q_coeff * q_diff.sum()  # not squared: the reference's device code
    return total


def quat_from_rpy64(r, p, y):
    """yaw about z, then pitch about y, then roll about x (body to world)"""
    half = lambda a, axis: np.concatenate([[np.cos(a / 2)], np.sin(a / 2) * np.eye(3)[axis]])
    return quat_mul64(quat_mul64(half(y, 2), half(p, 1)), half(r, 0))


def random_states(n, seed, flip_w=True):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (n, 13))
    x[:, 6:10] /= np.linalg.norm(x[:, 6:10], axis=1, keepdims=True)
    if not flip_w:
        x[:, 6:10] *= np.sign(x[:, 6:7])
    return x.astype(np.float32)


def _ulp_err(got, want64):
    """tests/test_det_math.py's measure"""
    want = want64.astype(np.float32)
    ulp = np.maximum(np.abs(np.spacing(want)).astype(np.float64), 1.4e-45)
    return np.abs(got.astype(np.float64) - want64) / ulp


# ------------------------------------------------------------------ configurations -------------------------------------
def quadrotor_cfg(K=192, T=7, D=1, use_euler=True, lambda_=2.0, num_iters=1):
    """a tilted, moving vehicle with q_w < 0 at the start, a goal away from it and sampler noise wide enough in thrust
    (std 12 N around a mean near both ends of [0, 36]) that samples leave the range on both sides"""
    cost = m.QuadrotorQuadraticCostParams()
    cost.s_goal[:] = [0.5, -0.3, 1.0, 0, 0, 0] + list(quat_from_rpy64(0.1, -0.2, 0.4).astype(np.float32)) + [0, 0, 0]
    cost.x_coeff, cost.v_coeff, cost.w_coeff = 40.0, 15.0, 0.5
    cost.roll_coeff, cost.pitch_coeff, cost.yaw_coeff, cost.q_coeff = 15.0, 12.0, 9.0, 7.0
    cost.use_euler = int(use_euler)
    cost.terminal_cost_coeff = 3.0
    q0 = -quat_from_rpy64(0.3, 0.2, -0.5)  # the same attitude on the q_w < 0 sheet
    x0 = np.concatenate([[0.1, 0.2, 0.8], [0.3, -0.1, 0.2], q0, [0.2, -0.4, 0.1]]).astype(np.float32)
    assert x0[6] < 0
    return dict(model="quadrotor", K=K, T=T, D=D, dt=0.02, lambda_=lambda_, alpha=0.1, num_iters=num_iters,
                dyn=m.QuadrotorDynamicsParams(1.3), cost=cost, ranges=None, std_dev=[0.5, 0.5, 0.5, 12.0],
                control_cost_coeff=[2.0, 2.0, 2.0, 0.3], x0=x0, oracle=make_quadrotor_oracle)


def make_quadrotor_oracle(cfg):
    o = qo.QuadrotorOracle(cfg["K"], cfg["T"], cfg["D"], cfg["dt"], cfg["lambda_"], cfg["alpha"], cfg["num_iters"])
    o.set_dynamics_params(cfg["dyn"])
    o.set_cost_params(cfg["cost"])
    if cfg["ranges"] is not None:
        o.set_control_ranges(cfg["ranges"])
    o.set_sampler(cfg["std_dev"], cfg["control_cost_coeff"], cfg.get("pure_pct", 0.01), cfg.get("decay", 1.0))
    return o


def nominal_control(T, thrust_pattern=True):
    """thrust = GRAVITY as the issue's initial sequence; with thrust_pattern, steps near both ends of [0, 36] too"""
    u = np.zeros((T, 4), np.float32)
    u[:, 3] = GRAVITY
    if thrust_pattern:
        u[1::3, 3] = 2.0
        u[2::3, 3] = 33.0
        u[:, 0] = 0.1
    return u


# ------------------------------------------------------------------ CPU: det::atan2 ------------------------------------
def test_det_atan2_accuracy_and_edges():
    """det::atan2 against float64 numpy.arctan2 on 10^6 points over the four quadrants (angles uniform in (-pi, pi], both
    magnitudes log-uniform over 1e-3 .. 1e3, so every ratio from 1e-6 to 1e6 occurs) within tests/test_det_math.py's bar for
    det::atan, 3 ulp.  Measured maximum: 2.683 ulp.  Then the axes, the signed zeros, equal magnitudes, huge / tiny and NaN."""
    rng = np.random.default_rng(14)
    ang = rng.uniform(-np.pi, np.pi, 1_000_000)
    y = (np.sin(ang) * np.exp(rng.uniform(np.log(1e-3), np.log(1e3), ang.size))).astype(np.float32)
    x = (np.cos(ang) * np.exp(rng.uniform(np.log(1e-3), np.log(1e3), ang.size))).astype(np.float32)
    got = qo.det_atan2(y, x)
    want = np.arctan2(y.astype(np.float64), x.astype(np.float64))
    for quadrant in ((x > 0) & (y > 0), (x < 0) & (y > 0), (x < 0) & (y < 0), (x > 0) & (y < 0)):
        assert quadrant.sum() > 200_000
    err = _ulp_err(got, want).max()
    print("det::atan2 max error %.3f ulp" % err)
    assert err <= 3.0, err

    pi, z, inf = np.float32(np.pi), np.float32(0.0), np.float32(np.inf)
    half, quarter = np.float32(np.pi / 2), np.float32(np.pi / 4)
    edge = [  # (y, x, expected) — libm's table
        (z, 1.0, z), (-z, 1.0, -z), (z, -1.0, pi), (-z, -1.0, -pi), (z, z, z), (-z, z, -z), (z, -z, pi), (-z, -z, -pi),
        (1.0, z, half), (1.0, -z, half), (-1.0, z, -half), (-1.0, -z, -half),
        (1.0, 1.0, quarter), (-3.5, 3.5, -quarter), (inf, inf, quarter), (-inf, inf, -quarter),
        (1.0, inf, z), (-1.0, inf, -z), (1.0, -inf, pi), (-1.0, -inf, -pi), (inf, 1.0, half), (-inf, -1.0, -half),
        (1e-30, 1e30, z), (-1e-30, 1e30, -z), (1e30, 1e-30, half), (1e30, -1e-30, half), (1e-30, -1e30, pi),
    ]
    ys, xs, want = (np.array(c, np.float32) for c in zip(*edge))
    got = qo.det_atan2(ys, xs)
    assert np.array_equal(bits(got), bits(want)), list(zip(ys, xs, got, want))
    # 3 pi / 4 is built as pi - pi / 4: within an ulp of the rounded constant
    g = qo.det_atan2(np.array([5.0, -5.0, inf], np.float32), np.array([-5.0, -5.0, -inf], np.float32))
    assert np.abs(np.abs(g) - 3 * np.pi / 4).max() < 2.4e-7 and g[1] < 0
    assert np.isnan(qo.det_atan2([np.nan, 1.0, np.nan], [1.0, np.nan, np.nan])).all()


# ------------------------------------------------------------------ CPU: quaternion helpers ----------------------------
@pytest.mark.parametrize("which", ["plugin", "restatement"])
def test_quaternion_helpers(which):
    """the helpers the product ships (include/mppi_amd/plugin/math_utils.hpp, host forms, built by
    tests/quadrotor_oracle/plugin_math_host.hip) and, as a second opinion, the CPU restatement's own copies: the zero-rotation
    DCM is the identity, QuatSubtract(q, q) the identity quaternion, Quat2EulerNWU returns the roll / pitch / yaw a quaternion
    was built from; all nine DCM entries, the products with and without normalisation, the inverse and the rate against float64"""
    h = qo.plugin_helpers() if which == "plugin" else qo.restatement_helpers()
    ident = np.array([1, 0, 0, 0], np.float32)
    assert np.array_equal(h.quat_to_dcm(ident), np.eye(3, dtype=np.float32))
    for q in random_states(20, 3)[:, 6:10]:
        d = h.quat_subtract(q, q)
        assert abs(d[0] - 1) <= 2.4e-7 and np.abs(d[1:]).max() <= 1.2e-7, (q, d)
        assert np.abs(h.quat_multiply(q, h.quat_inv(q)) - ident).max() <= 2.4e-7
        assert np.abs(h.quat_to_dcm(q) - rotation64(q)).max() <= 1e-6  # every entry: a sign error in any shows as ~1
        assert np.abs(h.omega_to_edot(0.3, -0.2, 0.5, q) - 0.5 * quat_mul64(q, [0, 0.3, -0.2, 0.5])).max() <= 1e-7
        q64 = q.astype(np.float64)
        # QuatInv is the conjugate over the NORM (the reference's, math_utils.h:188-199): a unit quaternion whatever the length
        assert np.abs(h.quat_inv(1.7 * q) - q64 * [1, -1, -1, -1]).max() <= 2e-7
    rng = np.random.default_rng(4)
    for r, p, y in np.column_stack([rng.uniform(-3.1, 3.1, 50), rng.uniform(-1.5, 1.5, 50), rng.uniform(-3.1, 3.1, 50)]):
        got = h.quat_to_euler(quat_from_rpy64(r, p, y).astype(np.float32))
        assert np.abs(got - [r, p, y]).max() <= 2e-5, ((r, p, y), got)  # d angle / d q is up to 1 / cos(pitch) ~ 14 at 1.5 rad
    # QuatMultiply normalises its product; the product of two unit quaternions against float64
    a, b = random_states(2, 5)[:, 6:10]
    assert np.abs(h.quat_multiply(a, b) - quat_mul64(a, b)).max() <= 3e-7
    if which == "plugin":
        # normalize = false: the plain Hamilton product of two quaternions that are not of unit length
        a2, b2 = (1.5 * a).astype(np.float32), (0.4 * b).astype(np.float32)
        want = quat_mul64(a2, b2)
        assert abs(np.linalg.norm(want) - 0.6) < 1e-6
        assert np.abs(h.quat_multiply(a2, b2, normalize=False) - want).max() <= 2e-7
        assert np.array_equal(h._call(7, (a,), 3), h.quat_to_dcm(a)[:, 2])  # Quat2DCMColumn3 is Quat2DCM's third column


def test_plugin_helpers_equal_restatement_bitwise():
    """the product's host forms and the restatement's copies on the same inputs, bit for bit — the kernels are then held to the
    restatement at 0 ulp on the GPU"""
    hp, hr = qo.plugin_helpers(), qo.restatement_helpers()
    qs = random_states(40, 8)[:, 6:10]
    for q, q2 in zip(qs[:20], qs[20:]):
        assert np.array_equal(bits(hp.quat_multiply(q, q2)), bits(hr.quat_multiply(q, q2)))
        assert np.array_equal(bits(hp.quat_inv(q)), bits(hr.quat_inv(q)))
        assert np.array_equal(bits(hp.quat_subtract(q, q2)), bits(hr.quat_subtract(q, q2)))
        assert np.array_equal(bits(hp.quat_to_euler(q)), bits(hr.quat_to_euler(q)))
        assert np.array_equal(bits(hp.quat_to_dcm(q)), bits(hr.quat_to_dcm(q)))
        assert np.array_equal(bits(hp.omega_to_edot(0.3, -0.2, 0.5, q)), bits(hr.omega_to_edot(0.3, -0.2, 0.5, q)))


def test_parameter_blocks_match_the_plugin_classes():
    """what a C or C++ caller hands to mppi_set_dynamics_params / mppi_set_cost_params: the plugin classes' default parameters,
    copied out of C++ as the POD blocks of model_params.h (plugin_math_host.hip static_asserts the sizes), are byte for byte the
    defaults of the Python mirrors; GRAVITY and the NaN guard of the cost class itself"""
    import ctypes as C
    L = qo.plugin_math()
    dyn, cost = m.QuadrotorDynamicsParams(5.0), m.QuadrotorQuadraticCostParams()
    cost.x_coeff = 9
    L.plugin_default_params(C.byref(dyn), C.byref(cost))
    assert bytes(dyn) == bytes(m.QuadrotorDynamicsParams()) and bytes(cost) == bytes(m.QuadrotorQuadraticCostParams())
    assert L.plugin_gravity() == GRAVITY
    assert L.plugin_nan_to_max_cost(float("nan")) == np.float32(1e16) and L.plugin_nan_to_max_cost(2.5) == 2.5


# ------------------------------------------------------------------ CPU: the reference's own tests ----------------------
def test_reference_held_values():
    """tests/dynamics/quadrotor_dynamics_tests.cu and tests/cost_functions/quadrotor_quadratic_cost_test.cu: the constructors'
    defaults, and their CPU-against-GPU comparisons (Eigen's Random() state and control in [-1, 1] with the quaternion
    normalised; default parameters for the derivative, mass 2.5 and dt 0.01 for the update, x_coeff = 5 for ControlCost) —
    the host side of those comparisons is the float64 restatement here, the device side the CPU restatement"""
    o = qo.QuadrotorOracle(4, 3)
    assert (o.S, o.C, o.O) == (13, 4, 13)
    lib = qo.lib()
    import ctypes as C
    s, c, out = C.c_int(), C.c_int(), C.c_int()
    lib.oracle_dims(o.h, C.byref(s), C.byref(c), C.byref(out))
    assert (s.value, c.value, out.value) == (13, 4, 13)
    dp, cp = m.QuadrotorDynamicsParams(), m.QuadrotorQuadraticCostParams()
    assert (dp.tau_roll, dp.tau_pitch, dp.tau_yaw, dp.mass) == (0.25, 0.25, 0.25, 1.0)
    assert list(cp.s_goal) == [0] * 6 + [1] + [0] * 6 and list(cp.control_cost_coeff) == [2.0] * 4
    assert cp.use_euler == 1 and cp.terminal_cost_coeff == 0 and cp.x_coeff == cp.q_coeff == cp.yaw_coeff == 1.0
    assert C.sizeof(dp) == 16 and C.sizeof(cp) == 4 * 27
    # default thrust range and zero control: a thrust of 50 is clamped to 36, -1 to 0; an empty slide tail is hover thrust
    x = np.zeros(13, np.float32)
    x[6] = 1
    assert o.model_step(x, [0, 0, 0, 50.0])[1][3] == 36.0 and o.model_step(x, [0, 0, 0, -1.0])[1][3] == 0.0
    assert o.model_step(x, [9.0, -9.0, 9.0, 1.0])[1][:3].tolist() == [9.0, -9.0, 9.0]
    o.set_nominal_control(nominal_control(3, False))
    o.vanilla_slide(3)
    assert np.array_equal(o.control(), nominal_control(3, False))

    x = random_states(1, 11)[0]
    u = np.random.default_rng(12).uniform(-1, 1, 4).astype(np.float32)
    xd = o.state_deriv(x, u)
    _, want = step64(x, u, 0.01)
    assert np.abs(xd - want).max() <= REL_TOL * np.abs(want).max()
    o.set_dynamics_params(m.QuadrotorDynamicsParams(2.5))
    xn = o.update_state(x, o.state_deriv(x, u), 0.01)
    want, _ = step64(x, u, 0.01, mass=2.5)
    assert np.abs(xn - want).max() <= REL_TOL * np.abs(want).max()
    assert abs(np.linalg.norm(xn[6:10].astype(np.float64)) - 1) < 2e-7 and xn[6] >= 0

    cp.x_coeff = 5
    o.set_cost_params(cp)
    want = cost64(x, cp)
    assert abs(o.state_cost(x)[0] - want) <= REL_TOL * want
    assert o.terminal_cost(x) == 0.0  # terminal_cost_coeff defaults to 0
    cp.terminal_cost_coeff = 2.5
    o.set_cost_params(cp)
    assert abs(o.terminal_cost(x) - 2.5 * want) <= REL_TOL * 2.5 * want


# ------------------------------------------------------------------ CPU: restatement against float64 -------------------
@pytest.mark.parametrize("use_euler", [True, False])
def test_step_and_cost_against_float64(use_euler):
    """the CPU restatement against the independent float64 one: random states with unit quaternions on both sheets (q_w < 0
    included), relative 1e-4 of the largest component (the reference's rollout tolerance)"""
    cfg = quadrotor_cfg(K=4, T=3, use_euler=use_euler)
    o = make_quadrotor_oracle(cfg)
    xs = random_states(300, 21)
    assert (xs[:, 6] < 0).sum() > 100
    us = np.random.default_rng(22).uniform(-1, 1, (300, 4)).astype(np.float32) * [2, 2, 2, 15] + [0, 0, 0, 18]
    worst_step = worst_cost = 0.0
    for x, u in zip(xs, us):
        xn, xd, y = o.model_step_full(x, u, 0.02)
        want_n, want_d = step64(x, u.astype(np.float32), 0.02, mass=1.3)
        worst_step = max(worst_step, np.abs(xn - want_n).max() / np.abs(want_n).max(), np.abs(xd - want_d).max() / np.abs(want_d).max())
        assert np.array_equal(y, xn) and xn[6] >= 0
        c, want_c = o.state_cost(x)[0], cost64(x, cfg["cost"])
        # without use_euler the attitude term is a signed sum: relative to the sum of the terms' magnitudes
        scale = abs(want_c) if use_euler else cost64(x, cfg["cost"]) + 2 * cfg["cost"].q_coeff * 2
        worst_cost = max(worst_cost, abs(c - want_c) / scale)
    print("step %.3g, cost %.3g relative" % (worst_step, worst_cost))
    assert worst_step <= REL_TOL and worst_cost <= REL_TOL


def test_nan_guard():
    """a NaN sum is MAX_COST_VALUE = 1e16, for the running and the terminal cost (the reference's arithmetic guard returns NaN)"""
    for use_euler in (True, False):
        cfg = quadrotor_cfg(K=4, T=3, use_euler=use_euler)
        o = make_quadrotor_oracle(cfg)
        for bad in (0, 4, 7, 11):
            y = cfg["x0"].copy()
            y[bad] = np.nan
            assert o.state_cost(y)[0] == np.float32(1e16), (use_euler, bad)
            assert o.terminal_cost(y) == np.float32(3.0) * np.float32(1e16)
        y = cfg["x0"].copy()
        y[6:10] = 0  # a zero quaternion: 1 / 0 * 0
        assert o.state_cost(y)[0] == np.float32(1e16)
        assert np.isfinite(o.state_cost(cfg["x0"])[0])


# ------------------------------------------------------------------ CPU: registration ----------------------------------
def test_registration(quadrotor):
    """the library lists the model and describes its shapes without a device"""
    assert "quadrotor" in m.list_models()
    qo.load_model(m)  # a second load is a no-op
    assert m.list_models().count("quadrotor") == 1
    d = m.describe_model("quadrotor")
    assert d["shapes"] == [(64, 1, 1), (64, 1, 2), (32, 4, 1), (16, 1, 1)] and d["pipeline"] and not d["rmppi"]
    assert d["replicated_lane_shapes"] == []
    assert m.describe_model("quadrotor", m.MPPI_SAMPLER_COLORED) is None


@pytest.mark.gpu
def test_colored_and_robust_are_refused(gpu, quadrotor):
    """marked gpu because mppi_create looks for a device before it looks at the model: both controllers are refused with a
    message, and no handle comes back"""
    with pytest.raises(m.MPPIError) as e:
        m.ColoredMPPIController("quadrotor", 64, 8, 0.01, 1.0)
    assert e.value.status == m.MPPI_ERR_UNSUPPORTED
    assert str(e.value).endswith("mppi_create: model 'quadrotor' has no colored-noise instantiation"), str(e.value)
    with pytest.raises(m.MPPIError) as e:
        m.RobustMPPIController("quadrotor", 288, 8, 0.01, 1.0)
    assert e.value.status == m.MPPI_ERR_UNSUPPORTED
    assert str(e.value).endswith("mppi_create: model 'quadrotor' is not instantiated for Robust MPPI"), str(e.value)


# ------------------------------------------------------------------ GPU: every shape, both families ---------------------
# every registered one-system shape as tests/kernel_forms.py chooses the forms: fused always, the role pipeline where
# pipeline_family() names one — (64, 1, 1) (test_forms_follow_kernel_forms holds this list to that rule)
FORMS = [("fused64x1x1", (64, 1, 1), m.MPPI_KERNEL_FUSED), ("pipeline64x1x1", (64, 1, 1), m.MPPI_KERNEL_PIPELINE),
         ("fused32x4x1", (32, 4, 1), m.MPPI_KERNEL_FUSED), ("fused16x1x1", (16, 1, 1), m.MPPI_KERNEL_FUSED)]


def test_forms_follow_kernel_forms(quadrotor):
    from kernel_forms import pipeline_family
    d = m.describe_model("quadrotor")
    want = []
    for sh in d["shapes"]:
        if sh[2] == 1:
            want.append(("fused%dx%dx%d" % sh, sh, m.MPPI_KERNEL_FUSED))
            if pipeline_family(d, sh):
                want.append(("pipeline%dx%dx%d" % sh, sh, m.MPPI_KERNEL_PIPELINE))
    assert want == FORMS
    assert pipeline_family(d, (64, 1, 2)) == "pipeline"


_REFERENCE = {}


def _reference_run(K, T, use_euler):
    """two consecutive calls of the CPU restatement with a slide between, computed once per (K, T, use_euler) and shared"""
    key = (K, T, use_euler)
    if key not in _REFERENCE:
        cfg = quadrotor_cfg(K=K, T=T, use_euler=use_euler)
        o = make_quadrotor_oracle(cfg)
        o.set_nominal_control(nominal_control(T))
        eps = [host_noise(1, K, T, 4, seed=K + T + i) for i in range(2)]
        x1 = o.model_step(cfg["x0"], nominal_control(T)[0])[0]
        calls = []
        for i, x in enumerate((cfg["x0"], x1)):
            mean = o.control().copy()
            o.vanilla_compute_control(x, 1, eps[i])
            calls.append(dict(x=x, eps=eps[i], mean=mean, costs=o.costs().copy(), control=o.control().copy(), samples=o.samples().copy()))
            o.vanilla_slide(1)
        # the inputs do what the issue asks of them: thrust samples below 0 and above 36 before the clamp, q_w < 0 at the start
        raw = o.set_gaussian_controls(nominal_control(T)[None], eps[0], 1, 0)[0, :, :, 3]
        assert (raw < 0).any() and (raw > 36).any() and cfg["x0"][6] < 0
        assert calls[0]["samples"][..., 3].min() == 0.0 and calls[0]["samples"][..., 3].max() == 36.0
        for c in calls:
            c["costs"].setflags(write=False)
        _REFERENCE[key] = calls
    return _REFERENCE[key]


_COSTS_64x1x1 = {}


@pytest.mark.gpu
@pytest.mark.parametrize("use_euler", [True, False], ids=["euler", "quat"])
@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_every_shape_and_family_against_restatement(gpu, quadrotor, form, use_euler):
    """K = 192 (three blocks of 64) and K = 100 (a partial block), T = 7 and 33 (below and above one sample group, no multiple
    of it): trajectory costs 0 ulp, clamped samples written back 0 ulp, u* within 1e-5, over two calls with a slide between
    (the second call's mean is the restatement's slid u*, which the engine's own has just been held to within 1e-5)"""
    name, shape, variant = form
    for K, T in ((192, 7), (100, 33)):
        calls = _reference_run(K, T, use_euler)
        cfg = quadrotor_cfg(K=K, T=T, use_euler=use_euler)
        eng = make_engine(cfg, block_x=shape[0], block_y=shape[1], kernel_variant=variant, save_samples=True)
        try:
            eng.updateImportanceSampler(nominal_control(T))
            for i, c in enumerate(calls):
                tag = "%s K=%d T=%d call %d" % (name, K, T, i)
                if i > 0:
                    # the slid u* is the next mean.  The engine's differs from the restatement's in the last bits (its merge
                    # adds the weighted samples in another order), and samples drawn around another mean are other samples:
                    # hold the slid sequence to the u* bar, then start both sides from the same mean
                    assert np.abs(eng.getControlSeq() - c["mean"]).max() <= U_TOL, tag
                    eng.updateImportanceSampler(c["mean"])
                eng.injectNoise(c["eps"])
                eng.computeControl(c["x"], 1)
                info = eng.getLaunchInfo()
                assert info["block"] == shape and info["family"] == ("fused" if variant == m.MPPI_KERNEL_FUSED else "pipeline"), (tag, info)
                costs = eng.getSampledCostSeq()
                dc = int(ulp_diff(costs, c["costs"]).max())
                du = float(np.abs(eng.getControlSeq() - c["control"]).max())
                dv = int(ulp_diff(eng.getSampledControls(), c["samples"]).max())
                print("%s: costs %d ulp, samples %d ulp, u* %.3g" % (tag, dc, dv, du))
                assert dc == 0, "%s: costs differ by up to %d ulp" % (tag, dc)
                assert dv == 0, "%s: clamped samples differ by up to %d ulp" % (tag, dv)
                assert du <= U_TOL, "%s: u* differs by %g" % (tag, du)
                # (32,4,1) and every other form give (64,1,1)'s costs bit for bit: the race-free updateState
                first = _COSTS_64x1x1.setdefault((K, T, use_euler, i), costs.copy())
                assert np.array_equal(bits(costs), bits(first)), tag
                eng.slideControlSequence(1)
        finally:
            eng.close()


@pytest.mark.gpu
def test_four_lane_form_equals_one_lane_form_bitwise(gpu, quadrotor):
    """Shape<32,4,1> against Shape<64,1,1> directly (the race-free claim of QuadrotorDynamics::updateState): costs and clamped
    samples bit for bit; the re-rolled state trajectory keeps its quaternion on the q_w >= 0 sheet at unit length"""
    cfg = quadrotor_cfg(K=192, T=33)
    eps = host_noise(1, 192, 33, 4, seed=9)
    got = []
    for bx, by in ((64, 1), (32, 4)):
        eng = make_engine(cfg, block_x=bx, block_y=by, kernel_variant=m.MPPI_KERNEL_FUSED, save_samples=True)
        eng.updateImportanceSampler(nominal_control(33))
        eng.injectNoise(eps)
        eng.computeControl(cfg["x0"], 1)
        assert eng.getLaunchInfo()["block"] == (bx, by, 1)
        got.append((eng.getSampledCostSeq(), eng.getSampledControls(), eng.getControlSeq(), eng.getTargetStateSeq()))
        eng.close()
    (c1, v1, u1, x1), (c4, v4, u4, x4) = got
    assert np.array_equal(bits(c1), bits(c4)) and np.array_equal(bits(v1), bits(v4))
    # u* is merged per block, and the two shapes cut K into other blocks: the standing bar, not bits; the trajectories follow u*
    assert np.abs(u1 - u4).max() <= U_TOL and np.abs(x1 - x4).max() <= 1e-5
    xs = got[0][3]
    assert (xs[1:, 6] >= 0).all() and np.abs(np.linalg.norm(xs[:, 6:10].astype(np.float64), axis=1) - 1).max() < 3e-7


# ------------------------------------------------------------------ GPU: Tube ------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("variant", [m.MPPI_KERNEL_FUSED, m.MPPI_KERNEL_PIPELINE], ids=["fused", "pipeline"])
def test_tube(gpu, quadrotor, variant):
    """Shape<64,1,2> at K = 128, T = 20: the first call starts the nominal system at the actual state, so both systems' costs
    are identical; costs, u* and nominal u* against the restatement's Tube computeControl"""
    cfg = quadrotor_cfg(K=128, T=20, D=2)
    eps = host_noise(1, 128, 20, 4, seed=5)
    o = make_quadrotor_oracle(cfg)
    o.set_nominal_control(nominal_control(20))
    o.tube_compute_control(cfg["x0"], 1, eps)
    eng = make_engine(cfg, block_x=64, block_y=1, kernel_variant=variant, save_samples=True)
    try:
        eng.updateImportanceSampler(nominal_control(20))
        eng.injectNoise(eps)
        eng.computeControl(cfg["x0"], 1)
        assert eng.getLaunchInfo()["block"] == (64, 1, 2)
        costs = eng.getSampledCostSeq()
        assert np.array_equal(bits(costs[0]), bits(costs[1]))
        assert int(ulp_diff(costs, o.costs()).max()) == 0
        assert np.abs(eng.getControlSeq() - o.control()).max() <= U_TOL
        assert np.abs(eng.getNominalControlSeq() - o.nominal_control()).max() <= U_TOL
    finally:
        eng.close()


# ------------------------------------------------------------------ GPU: the other compiled forms ----------------------
@pytest.mark.gpu
@pytest.mark.parametrize("variant", [m.MPPI_KERNEL_FUSED, m.MPPI_KERNEL_PIPELINE], ids=["fused", "pipeline"])
def test_rows_in_hbm_forms(gpu, quadrotor, variant):
    """MPPI_AMD_ROWS_IN_HBM=1: the sample rows in HBM instead of LDS, the forms a long horizon runs, at K = 100, T = 33"""
    from kernel_forms import env_override
    K, T = 100, 33
    c = _reference_run(K, T, True)[0]
    cfg = quadrotor_cfg(K=K, T=T)
    with env_override(MPPI_AMD_ROWS_IN_HBM="1"):
        eng = make_engine(cfg, block_x=64, block_y=1, kernel_variant=variant, save_samples=True)
    try:
        eng.updateImportanceSampler(nominal_control(T))
        eng.injectNoise(c["eps"])
        eng.computeControl(c["x"], 1)
        info = eng.getLaunchInfo()
        assert info["rows_in_hbm"] and info["block"] == (64, 1, 1), info
        assert int(ulp_diff(eng.getSampledCostSeq(), c["costs"]).max()) == 0
        assert int(ulp_diff(eng.getSampledControls(), c["samples"]).max()) == 0
        assert np.abs(eng.getControlSeq() - c["control"]).max() <= U_TOL
    finally:
        eng.close()


@pytest.mark.gpu
def test_streamed_merge_form(gpu, quadrotor):
    """two iterations with in-kernel Philox noise on the (64,1,1) pipeline: the second launch merges the first one's block
    records in its sampler waves (the STREAM_MERGE instantiation, T C % 4 == 0).  u* against the restatement on the same stream"""
    K, T = 200, 8
    cfg = quadrotor_cfg(K=K, T=T, num_iters=2)
    eng = make_engine(cfg, block_x=64, block_y=1, kernel_variant=m.MPPI_KERNEL_PIPELINE, save_samples=True)
    try:
        eng.updateImportanceSampler(nominal_control(T))
        eng.setSeed(PHILOX_SEED)
        eng.computeControl(cfg["x0"], 1)
        info = eng.getLaunchInfo()
        assert info["family"] == "pipeline" and info["streamed_merge"], info
        o = make_quadrotor_oracle(cfg)
        o.set_nominal_control(nominal_control(T))
        eps = np.stack([po.philox_normal(PHILOX_SEED, g, K, T, 4) for g in range(2)])
        o.vanilla_compute_control(cfg["x0"], 1, eps)
        du = float(np.abs(eng.getControlSeq() - o.control()).max())
        print("streamed merge: u* %.3g" % du)
        assert du <= U_TOL, du
    finally:
        eng.close()


@pytest.mark.gpu
def test_tube_auto_fold_form(gpu, quadrotor):
    """a Tube controller created without a block shape folds the two systems into the lanes of a wave, (32,1,2)"""
    cfg = quadrotor_cfg(K=128, T=20, D=2)
    eps = host_noise(1, 128, 20, 4, seed=5)
    o = make_quadrotor_oracle(cfg)
    o.set_nominal_control(nominal_control(20))
    o.tube_compute_control(cfg["x0"], 1, eps)
    eng = make_engine(cfg, kernel_variant=m.MPPI_KERNEL_AUTO, save_samples=True)
    try:
        eng.updateImportanceSampler(nominal_control(20))
        eng.injectNoise(eps)
        eng.computeControl(cfg["x0"], 1)
        info = eng.getLaunchInfo()
        assert info["family"] == "pipeline_fold" and info["block"] == (32, 1, 2), info
        assert int(ulp_diff(eng.getSampledCostSeq(), o.costs()).max()) == 0
        assert np.abs(eng.getControlSeq() - o.control()).max() <= U_TOL
        assert np.abs(eng.getNominalControlSeq() - o.nominal_control()).max() <= U_TOL
    finally:
        eng.close()


# ------------------------------------------------------------------ GPU: Philox, model step, atan2 ----------------------
@pytest.mark.gpu
def test_fused_philox_noise_reproduces_costs(gpu, quadrotor):
    """the in-kernel Philox draws at K = 128, T = 16: the same stream handed to the restatement reproduces the engine's costs
    (0 ulp).  mppi_sample_noise refuses this sampler ("draws inside the step loop; use mppi_philox_normal for its stream"), so
    the stream is taken from mppi_philox_normal, on the device, and held to the host evaluation of it"""
    cfg = quadrotor_cfg(K=128, T=16)
    eng = make_engine(cfg, save_samples=True)
    try:
        with pytest.raises(m.MPPIError) as e:
            eng.sampleNoise(1)
        assert e.value.status == m.MPPI_ERR_UNSUPPORTED
        assert str(e.value).endswith("noise dump: this sampler draws inside the step loop; use mppi_philox_normal for its stream")
        eps = m.philox_normal(PHILOX_SEED, 0, 128, 16, 4)
        assert np.array_equal(bits(eps), bits(po.philox_normal(PHILOX_SEED, 0, 128, 16, 4)))
        eng.updateImportanceSampler(nominal_control(16))
        eng.setSeed(PHILOX_SEED)
        eng.computeControl(cfg["x0"], 1)
        o = make_quadrotor_oracle(cfg)
        o.set_nominal_control(nominal_control(16))
        o.vanilla_compute_control(cfg["x0"], 1, eps[None])
        assert int(ulp_diff(eng.getSampledCostSeq(), o.costs()).max()) == 0
        assert np.abs(eng.getControlSeq() - o.control()).max() <= U_TOL
    finally:
        eng.close()


@pytest.mark.gpu
def test_model_step_equals_restatement_bitwise(gpu, quadrotor):
    """mppi_model_step: clamp, derivative, Euler step and renormalisation, on both quaternion sheets"""
    cfg = quadrotor_cfg(K=64, T=4)
    eng, o = make_engine(cfg), make_quadrotor_oracle(cfg)
    try:
        xs = random_states(64, 31)
        us = np.random.default_rng(32).uniform(-1, 1, (64, 4)).astype(np.float32) * [3, 3, 3, 30] + [0, 0, 0, 15]
        assert (xs[:, 6] < 0).any() and (us[:, 3] < 0).any() and (us[:, 3] > 36).any()
        for x, u in zip(xs, us.astype(np.float32)):
            ge, go = eng.modelStep(x, u), o.model_step(x, u)
            assert np.array_equal(bits(ge[0]), bits(go[0])), (x, u, ge[0], go[0])
            assert np.array_equal(bits(ge[1]), bits(go[1]))
            assert ge[0][6] >= 0
    finally:
        eng.close()


@pytest.mark.gpu
def test_det_atan2_device_equals_host_bitwise(gpu):
    """mppi_det_eval function 14 on 10^4 points of all four quadrants and the edge table's zeros, axes and infinities"""
    rng = np.random.default_rng(15)
    y = np.concatenate([rng.uniform(-10, 10, 9_980), [0.0, -0.0, 0.0, -0.0, 1, -1, 1, -1, np.inf, -np.inf, np.inf, 1e-30, 1e30, 3, -3,
                                                       2.5, 1e-40, 1e-40, -1e-44, np.nan]]).astype(np.float32)
    x = np.concatenate([rng.uniform(-10, 10, 9_980), [1.0, 1.0, -1.0, -1.0, 0.0, -0.0, -0.0, 0.0, np.inf, -np.inf, 1.0, 1e30, 1e-30, 3,
                                                       -3, np.inf, 1e-40, -1e-38, 1e-40, 1.0]]).astype(np.float32)
    assert y.size == 10_000
    assert np.array_equal(bits(m.det_atan2(y, x)), bits(qo.det_atan2(y, x)))


# ------------------------------------------------------------------ the reference's hover acceptance test --------------
HOVER_STEPS = 3000
HOVER_PREFIX = 60  # steps the CPU restatement runs (see test_hover_restatement_prefix)


def hover_cfg():
    """tests/controllers/vanilla_mppi_test.cu:160-256: K = 2048, T = 150, dt = 0.01, lambda = 4, alpha = 0.9, std_dev
    0.5 / 0.5 / 0.5 / 2.0, goal z = 1, coefficients 400 / 150 / 15 / 15 / 15 / 5, the cost's default control coefficients"""
    cost = m.QuadrotorQuadraticCostParams()
    cost.s_goal[2] = 1
    cost.x_coeff, cost.v_coeff = 400, 150
    cost.roll_coeff = cost.pitch_coeff = cost.yaw_coeff = 15
    cost.w_coeff = 5
    x0 = np.zeros(13, np.float32)
    x0[6] = 1
    return dict(model="quadrotor", K=2048, T=150, D=1, dt=0.01, lambda_=4.0, alpha=0.9, num_iters=1,
                dyn=m.QuadrotorDynamicsParams(), cost=cost, ranges=None, std_dev=[0.5, 0.5, 0.5, 2.0],
                control_cost_coeff=[2.0, 2.0, 2.0, 2.0], x0=x0, oracle=make_quadrotor_oracle)


def hover_loop(compute, control, step, slide, baseline, steps, trace=None):
    """vanilla_mppi_test.cu:268-306: the plant is the model's own step; returns (steps outside the 0.15 m ball, final state)"""
    x = hover_cfg()["x0"].copy()
    goal = np.array([0, 0, 1], np.float64)
    far = 0
    for i in range(steps):
        compute(x)
        u = control()[0].copy()
        assert np.isfinite(u).all() and np.isfinite(x).all() and np.isfinite(baseline()), i
        x = step(x, u)
        slide()
        far += np.linalg.norm(x[:3].astype(np.float64) - goal) > 0.15
        if trace is not None:
            trace.append((x.copy(), u, np.float32(baseline())))
    return far, x


def _oracle_hover(steps, trace=None):
    cfg = hover_cfg()
    o = make_quadrotor_oracle(cfg)
    o.set_nominal_control(nominal_control(cfg["T"], False))
    gen = [0]

    def compute(x):
        o.vanilla_compute_control(x, 1, po.philox_normal(SEED, gen[0], cfg["K"], cfg["T"], 4)[None])
        gen[0] += 1
    return hover_loop(compute, o.control, lambda x, u: o.model_step(x, u)[0], lambda: o.vanilla_slide(1),
                      lambda: float(o.stats()["baseline"][0]), steps, trace)


def _engine_hover(steps, trace=None, reference_order=False):
    cfg = hover_cfg()
    eng = make_engine(cfg)
    try:
        if reference_order:
            eng.setReductionMode(m.MPPI_REDUCTION_REFERENCE_ORDER)
        eng.updateImportanceSampler(nominal_control(cfg["T"], False))
        eng.setSeed(SEED)
        return hover_loop(lambda x: eng.computeControl(x, 1), eng.getControlSeq, lambda x, u: eng.modelStep(x, u)[0],
                          lambda: eng.slideControlSequence(1), lambda: float(eng.getStats().real_sys.baseline), steps, trace)
    finally:
        eng.close()


def test_hover_restatement_prefix():
    """HoverTest on the CPU restatement with the product's Philox stream.  One call of the restatement at K = 2048, T = 150
    takes about 0.1 s on one core, the literal 3000 steps five minutes — more than the CPU suite spends on all its
    double-integrator runs together — so the CPU side runs the first HOVER_PREFIX = 60 steps (6 s): nothing non-finite, the
    quaternion at unit length, and the vehicle on its way up (the smoothing filter sees a zero control history, so the first
    thrusts are below hover and z dips by 0.6 mm before it climbs).  The engine runs all 3000 (test_hover_engine) and is
    compared with this prefix bit for bit."""
    trace = []
    far, x = _oracle_hover(HOVER_PREFIX, trace)
    assert far == HOVER_PREFIX  # it starts 1 m below the goal
    z = np.array([t[0][2] for t in trace])
    assert z.min() > -1e-3 and z[-1] > 0.25 and (np.diff(z[5:]) > 0).all(), z
    assert abs(np.linalg.norm(x[6:10].astype(np.float64)) - 1) < 3e-7


@pytest.mark.gpu
def test_hover_engine(gpu, quadrotor):
    """Quadrotor_VanillaMPPI.HoverTest, literal parameters, 3000 closed-loop steps on the engine with its in-kernel Philox
    draws: fewer than 10 % of the steps outside the 0.15 m ball around (0, 0, 1), no NaN.  Measured on an MI355X: 137 of the 3000
    steps outside (4.6 %), 0.7 s wall time for the loop (printed).  Then the reference-order handle against
    the CPU restatement on the same stream over the first HOVER_PREFIX steps, bit for bit (plant state, control, baseline)."""
    t0 = time.perf_counter()
    far, x = _engine_hover(HOVER_STEPS)
    print("hover: %d of %d steps outside the ball, final position %s, %.1f s" % (far, HOVER_STEPS, x[:3], time.perf_counter() - t0))
    assert far / HOVER_STEPS < 0.1, far
    te, to = [], []
    _engine_hover(HOVER_PREFIX, te, reference_order=True)
    _oracle_hover(HOVER_PREFIX, to)
    assert len(te) == len(to)
    for i, (ra, rb) in enumerate(zip(te, to)):
        for j, (va, vb) in enumerate(zip(ra, rb)):
            assert np.array_equal(bits(va), bits(vb)), "HoverTest: step %d, item %d: %r != %r" % (i, j, va, vb)
