"""NLNDistribution through the reference's TEMPLATED host surface: examples/templated_cartpole_nln.hip instantiates
VanillaMPPIController<CartpoleDynamics, CartpoleQuadraticCost, DDPFeedback, T, K, NLNDistribution<...>> from the reference's
include paths (<mppi/sampling_distributions/nln/nln.cuh>), which registers the instantiation under MPPI_SAMPLER_NLN and creates
its handle with that sampler.  Built by tests/native_build.py, as every templated example is; the control sequence of
its first computeControl is held to the oracle fed the host-composed NLN noise of the same seed (tests/test_nln_sampler.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import mppi_generic_amd as m
import native_build as nb
import pyoracle as po
from common import U_TOL, cartpole_cfg, make_oracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "templated_cartpole_nln"
K, T, SIGMA, SEED = 1024, 30, 0.8, 42  # the example's ROLLOUTS, HORIZON, std_dev and the templated controllers' default seed


def _build():
    return nb.build_example(m, NAME, "-I" + os.path.join(REPO, "examples"))


def test_templated_nln_example_compiles_from_the_reference_include_paths():
    txt = open(os.path.join(REPO, "examples", NAME + ".hip")).read()
    incs = re.findall(r'#include [<"]([^>"]+)[>"]', txt)
    assert "mppi/sampling_distributions/nln/nln.cuh" in incs
    assert all(i.startswith("mppi/") or "/" not in i for i in incs), incs
    assert "mppi_amd" not in re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    blob = open(_build(), "rb").read()
    # the role-pipelined kernel was instantiated in the user's unit with the NLN sampler as its SAMPLING_T
    assert re.search(rb"rolloutPipelineKernel[A-Za-z0-9_]*NLNDistribution", blob) and b"gfx950" in blob


@pytest.mark.gpu
def test_templated_nln_example_equals_the_oracle(gpu):
    exe = _build()
    r = subprocess.run([exe, "40"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    u = np.array([float(v) for v in re.findall(r"^u\[\d+\] = (\S+)$", r.stdout, flags=re.M)], np.float32)
    assert u.size == T, r.stdout[-1000:]
    assert re.search(r"with the NLN sampler: 40 control steps, pole angle -?[\d.]+ rad", r.stdout), r.stdout[-500:]
    cfg = cartpole_cfg(K=K, T=T, lambda_=20.0)
    cfg["std_dev"] = [SIGMA]
    x0 = np.array([0.3, -0.2, 0.5, 0.1], np.float32)
    orc = make_oracle(cfg)
    z1 = po.philox_normal(SEED, 0, K, T, 1)
    z2 = po.philox_normal(SEED, 0, K, T, 1, stream=16)
    eps = (z1 * po.det_eval(2, (np.float32(SIGMA) * z2).astype(np.float32)).reshape(z1.shape)).astype(np.float32)
    orc.vanilla_compute_control(x0, 1, eps[None])
    du = float(np.abs(u - orc.control()[:, 0]).max())
    print("templated NLN example: u* %g from the oracle" % du)
    assert np.abs(u).max() > 1e-3 and du <= U_TOL, du
