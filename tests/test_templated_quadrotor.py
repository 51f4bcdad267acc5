"""examples/templated_quadrotor.hip: the reference's hover loop through the reference-named templated classes —
VanillaMPPIController<QuadrotorDynamics, QuadrotorQuadraticCost, DDPFeedback, 150, 2048, GaussianDistribution> on the reference's
include paths (<mppi/dynamics/quadrotor/quadrotor_dynamics.cuh>, <mppi/cost_functions/quadrotor/quadrotor_quadratic_cost.cuh>) —
builds with hipcc against the library and runs.  The unit instantiates the kernels of its own plugin types, so it needs no
registration of the model."""
import os
import re
import subprocess

import pytest

import mppi_generic_amd as m
import native_build as nb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "templated_quadrotor"


@pytest.fixture(scope="module")
def exe(lib):
    return nb.build_example(m, NAME)


def test_example_uses_the_reference_spellings_and_builds(exe):
    txt = open(os.path.join(REPO, "examples", NAME + ".hip")).read()
    incs = re.findall(r'#include [<"]([^>"]+)[>"]', txt)
    assert all(i.startswith("mppi/") or "/" not in i for i in incs), incs
    assert "mppi_amd" not in re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert os.access(exe, os.X_OK)


@pytest.mark.gpu
@pytest.mark.parametrize("lanes,steps", [(1, 3000), (4, 300)], ids=["one-lane-3000", "four-lanes-300"])
def test_hover_loop_runs(gpu, exe, lanes, steps):
    """the literal 3000 steps on one lane per rollout: fewer than 10 % outside the 0.15 m ball, the quaternion at unit length;
    300 steps on four lanes per rollout, dim3(64, 4, 1): the LDS + barrier form of the plugin contract, by which the vehicle is most of the way up"""
    r = subprocess.run([exe, str(steps), str(lanes)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    print(last)
    mt = re.search(r"(\d+) control steps in ([\d.]+) ms, (\d+) outside the ball, height ([-\d.]+) m, \|q\| ([\d.]+)", last)
    assert mt, last
    n, far, height, qn = int(mt.group(1)), int(mt.group(3)), float(mt.group(4)), float(mt.group(5))
    assert n == steps and abs(qn - 1) < 1e-5
    if steps == 3000:
        assert far / steps < 0.1 and abs(height - 1) < 0.15, last
    else:
        assert height > 0.7, last
