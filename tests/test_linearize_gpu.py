"""mppi_linearize / mppi_linearize_trajectory on the device (engine/linearize_kernel.hpp) against the host build of the same
model headers (tests/linearize_host), bit for bit; the refusals; non-interference with computeControl; the Python and C++
surfaces.  The host build itself is held to float64 in tests/test_linearize.py."""
import subprocess

import numpy as np
import pytest

import mppi_generic_amd as m
import native_build as nb
import linearize_cases as lc
import linearize_host as lh
from common import SEED, cartpole_cfg, di_cfg, host_noise, make_engine

pytestmark = pytest.mark.gpu
BLOB, _ = lc.autorally_weights()
# one lane / one wave; a last block one point short; full blocks only; a tail block of one point (blocks of 64 points for the
# lane-per-point models, of 16 for the network model)
SIZES = (1, 63, 64, 65)

# registered name -> (the Dynamics class as tests/linearize_host knows it, the sampler kinds it is registered for)
G, COL, NLN = m.MPPI_SAMPLER_GAUSSIAN, m.MPPI_SAMPLER_COLORED, m.MPPI_SAMPLER_NLN
REGISTRATIONS = {
    "cartpole": ("cartpole", (G, COL, NLN)),
    "double_integrator": ("double_integrator", (G, COL, NLN)),
    "double_integrator_robust": ("double_integrator", (G, COL, NLN)),
    "racer_dubins": ("racer_dubins", (G, COL)),
    "autorally_nn": ("autorally_nn", (G, COL, NLN)),
    "autorally_nn_robust": ("autorally_nn", (G,)),
    "quadrotor": ("quadrotor", (G,)),
    "quadrotor_map": ("quadrotor", (G,)),
}
CASES = [(name, kind) for name, (_, kinds) in REGISTRATIONS.items() for kind in kinds]


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


def _handle(name, kind, T=3):
    """a handle of the registration with the parameters the host build is given; nothing but the dynamics matters here"""
    _load_plugin_model(name)
    cls = m.ColoredMPPIController if kind == COL else m.VanillaMPPIController
    kw = {} if kind == COL else dict(sampler=kind)
    c = cls(name, 64, T, 0.02, 1.0, 0.0, 1, seed=SEED, **kw)
    model = REGISTRATIONS[name][0]
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
        host_kw = dict(weights=BLOB)
    return c, model, host_kw


@pytest.mark.parametrize("name,kind", CASES)
def test_device_equals_host_build_of_the_same_header(gpu, name, kind):
    c, model, host_kw = _handle(name, kind)
    assert c.hasComputeGrad()
    xs, us = lc.POINTS[model]()
    for n in SIZES:
        idx = np.arange(n) % xs.shape[0] if n > 1 else np.array([xs.shape[0] // 2])
        x, u = xs[idx], us[idx]
        A, B = c.computeGrad(x, u)
        A_h, B_h, _ = lh.host_grad(model, x, u, **host_kw)
        assert A.shape == A_h.shape and B.shape == B_h.shape and A.dtype == np.float32 and B.dtype == np.float32
        # 0 ulp; +0 and -0 are told apart too
        assert (A.view(np.uint32) == A_h.view(np.uint32)).all(), (name, n, np.abs(A - A_h).max())
        assert (B.view(np.uint32) == B_h.view(np.uint32)).all(), (name, n, np.abs(B - B_h).max())
    c.close()


def _bits_equal(a, b):
    return a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all()


@pytest.mark.parametrize("T", [3, 10])
def test_trajectory_equals_points_read_back_vanilla_cartpole(gpu, T):
    cfg = cartpole_cfg(K=64, T=T, soft=True)
    cfg["x0"] = np.array([0.0, 0.0, 0.5, 0.0], np.float32)
    eng = make_engine(cfg)
    eng.computeControl(cfg["x0"], 1)
    A, B = eng.computeGradTrajectory()
    assert A.shape == (T, 4, 4) and B.shape == (T, 4, 1)
    A_p, B_p = eng.computeGrad(eng.getTargetStateSeq(), eng.getControlSeq())
    assert _bits_equal(A, A_p) and _bits_equal(B, B_p)
    assert np.abs(A[:, 3, 2]).max() > 0  # the trajectory is a moving pole, not the origin
    with pytest.raises(m.MPPIError) as e:  # no nominal system on a Vanilla handle
        eng.computeGradTrajectory(system=1)
    assert e.value.status == m.MPPI_ERR_INVALID_ARG
    eng.close()


@pytest.mark.parametrize("T", [3, 10])
def test_trajectory_equals_points_read_back_tube_double_integrator(gpu, T):
    cfg = di_cfg(K=64, T=T, tube=True)
    eng = make_engine(cfg)
    eng.computeControl(cfg["x0"], 1)
    for system, xs, us in ((0, eng.getTargetStateSeq(), eng.getControlSeq()),
                           (1, eng.getNominalStateSeq(), eng.getNominalControlSeq())):
        A, B = eng.computeGradTrajectory(system=system)
        A_p, B_p = eng.computeGrad(xs, us)
        assert A.shape == (T, 4, 4) and B.shape == (T, 4, 2)
        assert _bits_equal(A, A_p) and _bits_equal(B, B_p)
    eng.close()


def test_trajectory_follows_the_system_asked_for(gpu):
    """the double integrator's Jacobians are constant, so the test above cannot tell system 0 from system 1: the cartpole on a
    Tube handle can — its two systems' trajectories differ once the actual state has left the nominal one"""
    cfg = cartpole_cfg(K=64, T=10, soft=True)
    cfg["D"] = 2
    eng = make_engine(cfg)
    eng.computeControl(np.array([0.0, 0.0, 0.5, 0.0], np.float32), 1)
    eng.computeControl(np.array([0.1, 0.3, 0.9, -0.5], np.float32), 1)
    out = []
    for system, xs, us in ((0, eng.getTargetStateSeq(), eng.getControlSeq()),
                           (1, eng.getNominalStateSeq(), eng.getNominalControlSeq())):
        A, B = eng.computeGradTrajectory(system=system)
        A_p, B_p = eng.computeGrad(xs, us)
        assert _bits_equal(A, A_p) and _bits_equal(B, B_p)
        out.append(A)
    assert not _bits_equal(out[0], out[1])
    eng.close()


def test_refusals(gpu):
    eng = make_engine(cartpole_cfg(K=64, T=3))
    with pytest.raises(m.MPPIError) as e:  # before the first computeControl
        eng.computeGradTrajectory()
    assert e.value.status == m.MPPI_ERR_STATE and "mppi_compute_control" in str(e.value)
    lib = m.load_library()
    z = np.zeros(16, np.float32)
    assert lib.mppi_linearize(eng._h, z[:4], z[:1], 0, z, z[:4]) == m.MPPI_ERR_INVALID_ARG  # n = 0
    assert b"at least 1" in lib.mppi_last_error(eng._h)
    assert lib.mppi_linearize(eng._h, z[:4], z[:1], -3, z, z[:4]) == m.MPPI_ERR_INVALID_ARG
    eng.close()
    # a model whose Dynamics class declares nothing
    unsupported = m.VanillaMPPIController("racer_dubins_elevation", 64, 3, 0.02, 1.0, 0.0, 1, seed=SEED)
    assert not unsupported.hasComputeGrad()
    S, C = unsupported.STATE_DIM, unsupported.CONTROL_DIM
    with pytest.raises(m.MPPIError) as e:
        unsupported.computeGrad(np.zeros((1, S)), np.zeros((1, C)))
    assert e.value.status == m.MPPI_ERR_UNSUPPORTED and "computeGrad" in str(e.value)
    with pytest.raises(m.MPPIError) as e:
        unsupported.computeGradTrajectory()
    assert e.value.status == m.MPPI_ERR_UNSUPPORTED
    unsupported.close()


def test_linearising_changes_nothing_a_controller_computes(gpu):
    cfg = cartpole_cfg(K=64, T=10, soft=True)
    eps = host_noise(2, cfg["K"], cfg["T"], 1)
    a, b = make_engine(cfg), make_engine(cfg)
    results = []
    for eng, linearise in ((a, True), (b, False)):
        eng.injectNoise(eps)
        eng.computeControl(cfg["x0"], 1)
        first = (eng.getControlSeq(), eng.getSampledCostSeq())
        if linearise:
            eng.computeGradTrajectory()
            eng.computeGrad(np.ones((65, 4), np.float32), np.ones((65, 1), np.float32))
        eng.slideControlSequence(1)
        eng.computeControl(cfg["x0"], 1)
        results.append(first + (eng.getControlSeq(), eng.getSampledCostSeq(), eng.getTargetStateSeq()))
        eng.close()
    for with_lin, without in zip(*results):
        assert _bits_equal(with_lin, without)


def _serial_sum(A, B):
    """float64 sum over the float32 entries, A then B, in order: what the C++ programs print"""
    total = 0.0
    for v in np.concatenate([A.reshape(-1), B.reshape(-1)]):
        total += float(v)
    return total


def _build_program(name):
    """compute_grad_host.cpp with g++ over the C ABI; compute_grad_templated.hip with hipcc, its kernels instantiated in the
    program's own translation unit (tests/native_build.py: build_probe_program)"""
    return nb.build_probe_program(m, name)


@pytest.fixture(scope="module")
def python_sums(gpu):
    """the sums of the Python methods on the controller both C++ programs set up: cartpole (1.5, 0.3, 0.7), K = 64, T = 10,
    controls in [-5, 5], sigma 5, the default seed; two fixed points, then the trajectory of one computeControl"""
    c = m.VanillaMPPIController("cartpole", 64, 10, 0.02, 0.25, 0.0, 1, seed=SEED)
    c.setDynamicsParams(m.CartpoleDynamicsParams(1.5, 0.3, 0.7))
    c.setControlRanges([[-5.0, 5.0]])
    c.setSamplingParams([5.0], [0.0], 0.01, 1.0)
    A, B = c.computeGrad(np.array([[0.3, -0.4, 0.7, 1.5], [-1.0, 0.2, 2.9, -2.0]], np.float32), np.array([[2.0], [-4.0]], np.float32))
    sums = dict(points=(A.size, B.size, _serial_sum(A, B)))
    c.computeControl(np.array([0.0, 0.0, 0.5, 0.0], np.float32), 1)
    A, B = c.computeGradTrajectory()
    sums["trajectory"] = (A.size, B.size, _serial_sum(A, B))
    c.close()
    return sums


def _program_lines(name):
    r = subprocess.run([_build_program(name)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = dict(l.split(" ", 1) for l in r.stdout.strip().splitlines())
    print(name, lines)
    return {k: v.split() for k, v in lines.items()}


def test_name_keyed_cpp_accessors_give_python_s_numbers(gpu, python_sums):
    """tests/probes/compute_grad_host.cpp: computeGrad / computeGradTrajectory of mppi_amd::VanillaMPPIController run the library's
    own kernels on the handle Python's controller has too — every sum is Python's, to the bit"""
    lines = _program_lines("compute_grad_host.cpp")
    n_a, n_b, total = python_sums["points"]
    assert [int(lines["points"][0]), int(lines["points"][1])] == [n_a, n_b] and float(lines["points"][2]) == total
    n_a, n_b, total = python_sums["trajectory"]
    assert [int(lines["trajectory"][0]), int(lines["trajectory"][1])] == [n_a, n_b]
    assert float(lines["trajectory"][2]) == total and float(lines["trajectory"][3]) == total and abs(total) > 1.0


def test_templated_cpp_accessors_give_python_s_numbers(gpu, python_sums):
    """tests/probes/compute_grad_templated.hip: VanillaMPPIController<CartpoleDynamics, ...>::computeGrad(state, control, A, B)
    and computeGradTrajectory, linearizeKernel<CartpoleDynamics> instantiated in the program's own unit.  At the two fixed points
    the sum is Python's to the bit (same header, same operations).  Along its own trajectory — the program's rollouts are its
    own, so the trajectory need not be Python's — the launch over the device-resident sequences sums to what computeGrad gives
    step by step at the sequences read back, to the bit."""
    lines = _program_lines("compute_grad_templated.hip")
    n_a, n_b, total = python_sums["points"]
    assert [int(lines["points"][0]), int(lines["points"][1])] == [n_a, n_b] and float(lines["points"][2]) == total
    assert [int(lines["trajectory"][0]), int(lines["trajectory"][1])] == list(python_sums["trajectory"][:2])
    assert float(lines["trajectory"][2]) == float(lines["trajectory"][3]) and abs(float(lines["trajectory"][2])) > 1.0
