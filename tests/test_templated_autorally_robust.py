"""examples/templated_autorally_robust.hip: the templated Vanilla and Robust controllers over NeuralNetModel<7,2,3> + ARRobustCost +
DDPFeedback, through the reference's include paths, on a synthetic network and four-channel map built in code.  It builds and
runs, and the first control sequence it prints is the registered model's ("autorally_nn_robust") at the same inputs."""
import os
import re
import subprocess

import numpy as np
import pytest

import mppi_generic_amd as m
import native_build as nb
import ar_robust_oracle as ar
from common import U_TOL
from restate64 import bits_equal

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "templated_autorally_robust"

# the example's literals
K, T, DT, LAMBDA = 1024, 20, 0.1, 20.0
MAP_BOUNDS = (-12.5, -9.7, 3.8, 6.0)
X0 = np.array([-12.05, 5.05, 0.0, 0.0, 4.0, -0.05, 0.0], np.float32)
STEPS = 3


def synthetic_network():
    i = np.arange(6 * 32 + 32 + 32 * 32 + 32 + 32 * 4 + 4, dtype=np.uint32)
    n = ((i * np.uint32(7919) + np.uint32(13)) % np.uint32(2001)).astype(np.int32) - 1000
    return n.astype(np.float32) * np.float32(0.0003)


def synthetic_map():
    r, c = np.meshgrid(np.arange(22), np.arange(28), indexing="ij")
    band = c + 3 * (r >= 16)
    c0 = np.where(band >= 20, 1.0, np.where(band >= 16, 0.6, 0.0))
    return ar.interleave([c0, 0.05 * c + 0.01 * r, 3.0 + 0.1 * c - 0.05 * r, 0.3 - 0.02 * c + 0.01 * r])


def example_cost_params():
    p = m.ARRobustCostParams()
    p.setTransformFromBounds(*MAP_BOUNDS)
    p.boundary_threshold, p.track_slop, p.heading_coeff, p.slip_coeff = 0.5, 1.0, 20, 10
    p.crash_coeff, p.max_slip_ang = 10000, 0.03
    return p


def example_gains():
    g = np.zeros((T, 7, 2), np.float32)
    g[:, 5, 0], g[:, 6, 0], g[:, 4, 1] = -0.25, 0.125, -0.5
    return g


@pytest.fixture(scope="module")
def robust_model(lib):
    """as in tests/test_ar_robust_cost.py: loaded for this module, taken out of the registry afterwards"""
    lib_ = ar.load_model(m)
    yield lib_
    assert lib_.mppi_unregister_model(b"autorally_nn_robust", m.MPPI_SAMPLER_GAUSSIAN) == m.MPPI_OK


@pytest.fixture(scope="module")
def exe(lib):
    return nb.build_example(m, NAME)


def test_example_uses_the_reference_spellings_and_builds(exe):
    txt = open(os.path.join(REPO, "examples", NAME + ".hip")).read()
    incs = re.findall(r'#include [<"]([^>"]+)[>"]', txt)
    assert all(i.startswith("mppi/") or "/" not in i for i in incs), incs
    assert "mppi/cost_functions/autorally/ar_robust_cost.cuh" in incs and "mppi/controllers/R-MPPI/robust_mppi_controller.cuh" in incs
    assert "mppi_amd" not in re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert os.access(exe, os.X_OK)
    # the literals of this file are the example's
    for literal in ("HORIZON = 20", "ROLLOUTS = 1024", "dt = 0.1f, lambda = 20.0f, alpha = 0.0f", "max_slip_ang = 0.03f",
                    "MAP_X_MIN = -12.5, MAP_X_MAX = -9.7, MAP_Y_MIN = 3.8, MAP_Y_MAX = 6.0", "(i * 7919u + 13u) % 2001u",
                    "value_function_threshold = 1000.0f"):
        assert literal in txt, literal
    # the synthetic inputs restated here are the example's: multiples of 0.0003 within [-0.3, 0.3], bands of 0 / 0.6 / 1
    w, t = synthetic_network(), synthetic_map()
    assert w.size == 1412 and abs(w).max() <= np.float32(0.3) and w[0] == np.float32(-987) * np.float32(0.0003)
    assert t.shape == (22, 28, 4) and set(np.unique(t[:, :, 0]).tolist()) == {0.0, np.float32(0.6), 1.0}


def _registered(cls, **kw):
    eng = cls("autorally_nn_robust", K, T, DT, LAMBDA, 0.0, 1, seed=42, **kw)
    eng.setCostParams(example_cost_params())
    eng.setModelBlob("dynamics_weights", synthetic_network())
    eng.setModelBlob("costmap", synthetic_map())
    eng.setControlRanges([[-0.99, 0.99], [-0.99, 0.65]])
    eng.setSamplingParams([0.3, 0.3], [0.2, 0.1], 0.01, 1.0)
    return eng


@pytest.mark.gpu
def test_example_runs_and_matches_the_registered_model(gpu, robust_model, exe):
    """the example's first control sequences (in-kernel Philox noise, seed 42) against handles on "autorally_nn_robust" with the
    same network, map, parameters and seed.  Vanilla: the templated controller's default form is the fused kernel on (64, 1, 1)
    with NeuralNetModel; the registered model asked for that shape runs the same kernel form, and u* is equal bit for bit.
    Robust: the templated instantiation has no replicated-lane form (one lane per rollout and system), the registered one runs
    its MFMA form on the role-pipelined Robust kernel: u* within 1e-5"""
    r = subprocess.run([exe, str(STEPS)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    seqs = {}
    for tag in ("vanilla", "robust"):
        rows = re.findall(r"^%s u\[(\d+)\] = (\S+) (\S+)$" % tag, r.stdout, flags=re.M)
        assert [int(a) for a, _, _ in rows] == list(range(T)), (tag, rows)
        seqs[tag] = np.array([[float(b), float(c)] for _, b, c in rows], np.float32)
        baseline = float(re.search(r"^%s baseline = (\S+)$" % tag, r.stdout, flags=re.M).group(1))
        assert np.isfinite(baseline) and baseline > 0 and np.isfinite(seqs[tag]).all() and np.abs(seqs[tag]).max() > 0, tag
    assert "MPPI: after %d steps" % STEPS in r.stdout and "Robust MPPI: after %d steps" % STEPS in r.stdout

    eng = _registered(m.VanillaMPPIController, block_x=64, block_y=1, kernel_variant=m.MPPI_KERNEL_FUSED)
    try:
        eng.computeControl(X0, 1)
        info = eng.getLaunchInfo()
        assert info["family"] == "fused" and info["block"] == (64, 1, 1), info
        du = float(np.abs(eng.getControlSeq() - seqs["vanilla"]).max())
        print("vanilla: u* %.3g from the registered model's" % du)
        assert bits_equal(eng.getControlSeq(), seqs["vanilla"]), du
    finally:
        eng.close()
    eng = _registered(m.RobustMPPIController)
    try:
        eng.setRMPPIParams(1000.0, 9, 32)
        eng.setFeedbackGains(example_gains())
        eng.updateImportanceSamplingControl(X0, 1)
        eng.computeControl(X0, 1)
        du = float(np.abs(eng.getControlSeq() - seqs["robust"]).max())
        print("robust: u* %.3g from the registered model's (%s)" % (du, eng.getLaunchInfo()["family"]))
        assert du <= U_TOL, du
    finally:
        eng.close()
