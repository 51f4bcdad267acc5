"""mppi_set_feedback_params / mppi_compute_feedback / mppi_compute_feedback_at on the device (engine/feedback_kernel.hpp) against
the host build of the same header (tests/feedback_host), bit for bit; the trajectory entry against the points entry; the in-place
install on a Robust handle against an upload; the refusals; non-interference with computeControl; the C++ surfaces.  The host
build itself is held to float64 in tests/test_feedback.py."""
import subprocess

import numpy as np
import pytest

import mppi_generic_amd as m
import native_build as nb
import feedback_host as fh
import linearize_cases as lc
import linearize_host as lh
from common import SEED, cartpole_cfg, di_cfg, host_noise, make_engine, rm_cfg

pytestmark = pytest.mark.gpu
BLOB, _ = lc.autorally_weights()
DT = 0.02
ACCEPTANCE_Q = np.diag([500.0, 500.0, 100.0, 100.0]).astype(np.float32)

# registered name -> the Dynamics class as tests/linearize_host knows it: every registration with a computeGrad
REGISTRATIONS = {
    "cartpole": "cartpole",                        # C = 1: the scalar solve
    "double_integrator": "double_integrator",
    "double_integrator_robust": "double_integrator",
    "racer_dubins": "racer_dubins",
    "autorally_nn": "autorally_nn",
    "autorally_nn_robust": "autorally_nn",
    "quadrotor": "quadrotor",                      # S = 13, C = 4: several entries per lane, the full-depth LDL^T
    "quadrotor_map": "quadrotor",
}


def _bits_equal(a, b):
    return a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all()


def _load_plugin_model(name):
    if name == "quadrotor":
        import quadrotor_oracle
        quadrotor_oracle.load_model(m)
    elif name == "quadrotor_map":
        import quadrotor_map_oracle
        quadrotor_map_oracle.load_model(m)
    elif name == "autorally_nn_robust":
        import ar_robust_oracle
        ar_robust_oracle.load_model(m)


def _handle(name, T):
    _load_plugin_model(name)
    c = m.VanillaMPPIController(name, 64, T, DT, 1.0, 0.0, 1, seed=SEED)
    model = REGISTRATIONS[name]
    host_kw = {}
    if model == "cartpole":
        p = lc.CARTPOLE_PARAMS[1]
        c.setDynamicsParams(m.CartpoleDynamicsParams(*[float(v) for v in p]))
        host_kw = dict(params=p)
    elif model == "quadrotor":
        p = lc.QUADROTOR_PARAMS[1]
        q = m.QuadrotorDynamicsParams()
        q.tau_roll, q.tau_pitch, q.tau_yaw, q.mass = [float(v) for v in p]
        c.setDynamicsParams(q)
        host_kw = dict(params=p)
    elif model == "autorally_nn":
        c.setModelBlob("dynamics_weights", BLOB)
    return c, model, host_kw


def _horizons(model):
    """one backward step; two; one past the linearise block boundary (64 points for lane-per-point models, 16 for the network)"""
    return (2, 3, 17) if model == "autorally_nn" else (2, 3, 65)


@pytest.mark.parametrize("name", sorted(REGISTRATIONS))
def test_device_equals_host_build_of_the_same_header(gpu, name):
    for T in _horizons(REGISTRATIONS[name]):
        c, model, host_kw = _handle(name, T)
        xs, us = lc.POINTS[model]()
        idx = np.arange(T) % xs.shape[0]
        x, u = xs[idx], us[idx]
        if model == "autorally_nn":
            A, B = c.computeGrad(x, u)  # the network's Jacobians from the same handle
        else:
            A, B, _ = lh.host_grad(model, x, u, **host_kw)
        weights = [dict()]
        if model == "double_integrator":
            weights.append(dict(Q=ACCEPTANCE_Q))
        for w in weights:
            c.setFeedbackParams(Q=w.get("Q"))
            G = c.computeFeedbackAt(x, u)
            G_h, ok, step = fh.host_gains(A, B, DT, **w)
            assert ok and step == -1
            assert G.shape == G_h.shape == (T, c.STATE_DIM, c.CONTROL_DIM) and G.dtype == np.float32
            assert not G[T - 1].any()
            # 0 ulp; +0 and -0 are told apart too
            assert _bits_equal(G, G_h), (name, T, np.abs(G - G_h).max())
        c.close()


@pytest.mark.parametrize("T", [3, 10])
def test_trajectory_entry_equals_points_entry_vanilla_cartpole(gpu, T):
    cfg = cartpole_cfg(K=64, T=T, soft=True)
    cfg["x0"] = np.array([0.0, 0.0, 0.5, 0.0], np.float32)
    eng = make_engine(cfg)
    eng.computeControl(cfg["x0"], 1)
    G = eng.computeFeedback()
    G_p = eng.computeFeedbackAt(eng.getTargetStateSeq(), eng.getControlSeq())
    assert G.shape == (T, 4, 1) and _bits_equal(G, G_p)
    assert np.abs(G[:T - 1]).max() > 0 and not G[T - 1].any()
    eng.close()


def test_trajectory_entry_equals_points_entry_tube_double_integrator(gpu):
    cfg = di_cfg(K=64, T=10, tube=True)
    eng = make_engine(cfg)
    eng.setFeedbackParams(Q=ACCEPTANCE_Q)
    eng.computeControl(cfg["x0"], 1)
    for system, xs, us in ((0, eng.getTargetStateSeq(), eng.getControlSeq()),
                           (1, eng.getNominalStateSeq(), eng.getNominalControlSeq())):
        G = eng.computeFeedback(system=system)
        G_p = eng.computeFeedbackAt(xs, us)
        assert G.shape == (10, 4, 2) and _bits_equal(G, G_p)
    eng.close()


def _robust(cfg):
    eng = m.RobustMPPIController(cfg["model"], cfg["K"], cfg["T"], cfg["dt"], cfg["lambda_"], cfg["alpha"], cfg["num_iters"], seed=SEED)
    eng.setCostParams(cfg["cost"])
    eng.setControlRanges(cfg["ranges"])
    eng.setSamplingParams(cfg["std_dev"], cfg["control_cost_coeff"], 0.01, 1.0)
    eng.setRMPPIParams(1000.0, 9, 32)
    return eng


def test_in_place_install_equals_upload(gpu):
    """two Robust double-integrator handles, same seed and injected noise: A computes its gains and installs them on the device,
    B is handed A's gains through mppi_set_feedback_gains; the next computeControl is the same on both, bit for bit"""
    cfg = rm_cfg("di", K=512, T=20)
    S, Cd, T = 4, 2, cfg["T"]
    g0 = np.random.default_rng(1).uniform(-0.3, 0.3, (T, S, Cd)).astype(np.float32)
    eps = host_noise(2, cfg["K"], T, Cd)
    a, b = _robust(cfg), _robust(cfg)
    x = cfg["x0"]
    for eng in (a, b):
        eng.setFeedbackParams(Q=ACCEPTANCE_Q)
        eng.setFeedbackGains(g0)
        eng.injectNoise(eps)
        eng.updateImportanceSamplingControl(x, 1)
        eng.computeControl(x, 1)
    out = a.computeFeedback(system=1)
    assert np.abs(out[:T - 1]).max() > 0 and not _bits_equal(out, g0)
    b.setFeedbackGains(out)
    x2 = x + np.array([0.05, -0.03, 0.1, -0.05], np.float32)
    results = []
    for eng in (a, b):
        eng.computeControl(x2, 1)
        results.append((eng.getControlSeq(), eng.getNominalControlSeq(), eng.getSampledCostSeq(), eng.getTargetStateSeq()))
        eng.close()
    for in_place, uploaded in zip(*results):
        assert _bits_equal(in_place, uploaded)


def test_robust_handle_without_gains_runs_after_compute_feedback_alone(gpu):
    cfg = rm_cfg("di", K=512, T=20)
    eng = _robust(cfg)
    with pytest.raises(m.MPPIError) as e:
        eng.computeControl(cfg["x0"], 1)
    assert e.value.status == m.MPPI_ERR_STATE and "gains" in str(e.value)
    with pytest.raises(m.MPPIError) as e:  # no trajectory of any kind yet
        eng.computeFeedback(system=1)
    assert e.value.status == m.MPPI_ERR_STATE
    eng.updateImportanceSamplingControl(cfg["x0"], 1)  # leaves the nominal trajectory the reference computes its first gains on
    G = eng.computeFeedback(system=1)
    G_p = eng.computeFeedbackAt(eng.getTargetStateSeq(), eng.getNominalControlSeq())
    assert _bits_equal(G, G_p)
    eng.computeControl(cfg["x0"], 1)
    assert np.isfinite(eng.getControlSeq()).all()
    eng.close()


def test_refusals(gpu):
    lib = m.load_library()
    eng = make_engine(cartpole_cfg(K=64, T=6))
    with pytest.raises(m.MPPIError) as e:  # before the first computeControl
        eng.computeFeedback()
    assert e.value.status == m.MPPI_ERR_STATE and "mppi_compute_control" in str(e.value)
    with pytest.raises(m.MPPIError) as e:
        eng.setFeedbackParams(num_iterations=2)
    assert e.value.status == m.MPPI_ERR_UNSUPPORTED and "ddp.h:129-162" in str(e.value) and "line search" in str(e.value)
    eng.computeControl(np.array([0.0, 0.0, 0.5, 0.0], np.float32), 1)
    with pytest.raises(m.MPPIError) as e:  # no nominal system on a Vanilla handle
        eng.computeFeedback(system=1)
    assert e.value.status == m.MPPI_ERR_INVALID_ARG
    x = np.zeros((6, 4), np.float32)
    u = np.zeros((6, 1), np.float32)
    g = np.full((6, 4, 1), -3.0, np.float32)
    assert lib.mppi_compute_feedback_at(eng._h, None, u.ctypes.data, g.ctypes.data) == m.MPPI_ERR_INVALID_ARG
    assert lib.mppi_compute_feedback_at(eng._h, x.ctypes.data, None, g.ctypes.data) == m.MPPI_ERR_INVALID_ARG
    assert b"null" in lib.mppi_last_error(eng._h) and (g == -3.0).all()
    assert lib.mppi_compute_feedback(eng._h, 0, None) == m.MPPI_OK  # gains_out may be null
    eng.close()
    unsupported = m.VanillaMPPIController("racer_dubins_elevation", 64, 3, 0.02, 1.0, 0.0, 1, seed=SEED)
    S, Cd = unsupported.STATE_DIM, unsupported.CONTROL_DIM
    with pytest.raises(m.MPPIError) as e:
        unsupported.computeFeedbackAt(np.zeros((3, S)), np.zeros((3, Cd)))
    assert e.value.status == m.MPPI_ERR_UNSUPPORTED and "computeGrad" in str(e.value)
    with pytest.raises(m.MPPIError) as e:
        unsupported.computeFeedback()
    assert e.value.status == m.MPPI_ERR_UNSUPPORTED
    unsupported.close()


def test_failed_pivot_is_reported_and_the_previous_gains_stay(gpu):
    """the model's own B cannot be made zero from outside, the weights can: R = 0, Q = 0 and Qf = 0 give quu = Bd^T 0 Bd = 0 at
    the first step of the pass, T - 2.  Handle b never asks for feedback; both end with the same next computeControl."""
    cfg = rm_cfg("di", K=512, T=20)
    T = cfg["T"]
    eps = host_noise(2, cfg["K"], T, 2)
    g0 = np.random.default_rng(2).uniform(-0.3, 0.3, (T, 4, 2)).astype(np.float32)
    a, b = _robust(cfg), _robust(cfg)
    results = []
    for eng, fail in ((a, True), (b, False)):
        eng.setFeedbackGains(g0)
        eng.injectNoise(eps)
        eng.updateImportanceSamplingControl(cfg["x0"], 1)
        eng.computeControl(cfg["x0"], 1)
        if fail:
            zero4, zero2 = np.zeros((4, 4), np.float32), np.zeros((2, 2), np.float32)
            eng.setFeedbackParams(Q=zero4, R=zero2, Q_f=zero4)
            with pytest.raises(m.MPPIError) as e:
                eng.computeFeedback(system=1)
            assert e.value.status == m.MPPI_ERR_NAN and "step %d" % (T - 2) in str(e.value)
            out = np.full((T, 4, 2), -3.0, np.float32)
            assert m.load_library().mppi_compute_feedback(eng._h, 1, out.ctypes.data) == m.MPPI_ERR_NAN
            assert (out == -3.0).all()
        eng.computeControl(cfg["x0"], 1)  # the gains set before are still installed and still work
        results.append((eng.getControlSeq(), eng.getSampledCostSeq()))
        eng.close()
    for failed, untouched in zip(*results):
        assert _bits_equal(failed, untouched)


def test_computing_feedback_changes_nothing_a_controller_computes(gpu):
    cfg = cartpole_cfg(K=64, T=10, soft=True)
    eps = host_noise(2, cfg["K"], cfg["T"], 1)
    a, b = make_engine(cfg), make_engine(cfg)
    results = []
    for eng, feedback in ((a, True), (b, False)):
        eng.injectNoise(eps)
        eng.computeControl(cfg["x0"], 1)
        first = (eng.getControlSeq(), eng.getSampledCostSeq())
        if feedback:
            eng.setFeedbackParams(Q=np.diag([5.0, 1.0, 20.0, 1.0]))
            eng.computeFeedback()
            eng.computeFeedbackAt(np.ones((10, 4), np.float32), np.ones((10, 1), np.float32))
        eng.slideControlSequence(1)
        eng.computeControl(cfg["x0"], 1)
        results.append(first + (eng.getControlSeq(), eng.getSampledCostSeq(), eng.getTargetStateSeq()))
        eng.close()
    for with_fb, without in zip(*results):
        assert _bits_equal(with_fb, without)


def _serial_sum(G):
    """float64 sum over the float32 entries in order: what the C++ programs print"""
    total = 0.0
    for v in G.reshape(-1):
        total += float(v)
    return total


def _build_program(name):
    """compute_feedback_host.cpp with g++ over the C ABI; compute_feedback_templated.hip with hipcc, its kernels instantiated in
    the program's own translation unit (tests/native_build.py: build_probe_program)"""
    return nb.build_probe_program(m, name)


POINTS_X = np.array([[0.3, -0.4, 0.7, 1.5], [-1.0, 0.2, 2.9, -2.0]], np.float32)
POINTS_U = np.array([[2.0], [-4.0]], np.float32)
PROBE_Q = np.diag([5.0, 1.0, 20.0, 2.0]).astype(np.float32)
PROBE_R = np.array([[0.5]], np.float32)
PROBE_QF = np.diag([3.0, 3.0, 3.0, 3.0]).astype(np.float32)


@pytest.fixture(scope="module")
def python_sums(gpu):
    """the sums of the Python methods on the controller both C++ programs set up: cartpole (1.5, 0.3, 0.7), K = 64, T = 10,
    controls in [-5, 5], sigma 5, the default seed, Q = diag(5, 1, 20, 2), R = 0.5, Q_f = 3 I; the two fixed points cycled over
    the horizon, then the trajectory of one computeControl"""
    c = m.VanillaMPPIController("cartpole", 64, 10, 0.02, 0.25, 0.0, 1, seed=SEED)
    c.setDynamicsParams(m.CartpoleDynamicsParams(1.5, 0.3, 0.7))
    c.setControlRanges([[-5.0, 5.0]])
    c.setSamplingParams([5.0], [0.0], 0.01, 1.0)
    c.setFeedbackParams(PROBE_Q, PROBE_R, PROBE_QF)
    idx = np.arange(10) % 2
    G = c.computeFeedbackAt(POINTS_X[idx], POINTS_U[idx])
    sums = dict(points=(G.size, _serial_sum(G)))
    c.computeControl(np.array([0.0, 0.0, 0.5, 0.0], np.float32), 1)
    G = c.computeFeedback()
    sums["trajectory"] = (G.size, _serial_sum(G))
    c.close()
    return sums


def _program_lines(name):
    r = subprocess.run([_build_program(name)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = dict(l.split(" ", 1) for l in r.stdout.strip().splitlines())
    print(name, lines)
    return {k: v.split() for k, v in lines.items()}


def test_name_keyed_cpp_accessors_give_python_s_numbers(gpu, python_sums):
    """tests/probes/compute_feedback_host.cpp: setFeedbackParams / computeFeedbackAt / computeFeedback of
    mppi_amd::VanillaMPPIController run the library's own kernels on the handle Python's controller has too — every sum is
    Python's, to the bit"""
    lines = _program_lines("compute_feedback_host.cpp")
    n, total = python_sums["points"]
    assert int(lines["points"][0]) == n and float(lines["points"][1]) == total and abs(total) > 1.0
    n, total = python_sums["trajectory"]
    assert int(lines["trajectory"][0]) == n and float(lines["trajectory"][1]) == total and float(lines["trajectory"][2]) == total


def test_templated_cpp_accessors_give_python_s_numbers(gpu, python_sums):
    """tests/probes/compute_feedback_templated.hip: DDPFeedback<CartpoleDynamics, 10>::setParams / computeFeedback and the
    controller's computeFeedback(state), ddpBackwardKernel<4, 1> instantiated in the program's own unit.  At the fixed points the
    sum is Python's to the bit.  Along its own trajectory — the program's rollouts are its own — the controller's
    computeFeedback(state) sums to what mppi_compute_feedback gives on the same handle, to the bit."""
    lines = _program_lines("compute_feedback_templated.hip")
    n, total = python_sums["points"]
    assert int(lines["points"][0]) == n and float(lines["points"][1]) == total
    assert int(lines["trajectory"][0]) == python_sums["trajectory"][0]
    assert float(lines["trajectory"][1]) == float(lines["trajectory"][2]) and abs(float(lines["trajectory"][1])) > 1.0
