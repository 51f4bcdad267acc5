"""examples/templated_quadrotor_volume.hip: the templated Vanilla controller over QuadrotorDynamics + QuadrotorVolumeCost, through the
reference's include paths, flies past a pillar described by a clearance volume.  It builds and runs, and the first control sequence
it prints is the registered model's ("quadrotor_volume") at the same inputs, bit for bit on the same kernel form."""
import os
import re
import subprocess

import numpy as np
import pytest

import mppi_generic_amd as m
import native_build as nb
import texture3d_oracle as t3
from restate64 import bits_equal

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "templated_quadrotor_volume"

# the example's literals
K, T, DT, LAMBDA = 256, 40, 0.02, 5.0
VOL_W, VOL_H, VOL_D, CELL = 16, 12, 6, 0.5
STEPS = 60


def pillar_volume():
    """max(0, 1 - distance / 1.5) to the axis at (2, 0), in float32 as the example computes it"""
    f = np.float32
    x = f(-2.0) + f(CELL) * (np.arange(VOL_W, dtype=np.float32) + f(0.5))
    y = f(-3.0) + f(CELL) * (np.arange(VOL_H, dtype=np.float32) + f(0.5))
    dx, dy = (x - f(2.0))[None, :], (y - f(0.0))[:, None]
    dist = np.sqrt(dx * dx + dy * dy, dtype=np.float32)
    layer = np.maximum(f(0.0), f(1.0) - dist / f(1.5)).astype(np.float32)
    return np.broadcast_to(layer[None], (VOL_D, VOL_H, VOL_W)).copy()


def example_cost_params():
    p = m.QuadrotorVolumeCostParams()
    p.s_goal[0:3] = [4.0, 0.25, 1.5]
    p.x_coeff, p.v_coeff, p.w_coeff = 40, 15, 5
    p.roll_coeff = p.pitch_coeff = p.yaw_coeff = 15
    p.volume_coeff, p.crash_threshold, p.crash_coeff = 200.0, 0.6, 1000.0
    return p


@pytest.fixture(scope="module")
def exe(lib):
    return nb.build_example(m, NAME)


def test_example_uses_the_reference_spellings_and_builds(exe):
    txt = open(os.path.join(REPO, "examples", NAME + ".hip")).read()
    incs = re.findall(r'#include [<"]([^>"]+)[>"]', txt)
    assert all(i.startswith("mppi/") or "/" not in i for i in incs), incs
    assert "mppi/utils/texture_helpers/three_d_texture_helper.cuh" in incs
    assert "mppi_amd" not in re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert os.access(exe, os.X_OK)
    # the literals of this file are the example's
    for literal in ("HORIZON = 40", "ROLLOUTS = 256", "dt = 0.02f, lambda = 5.0f, alpha = 0.0f", "VOL_WIDTH = 16, VOL_HEIGHT = 12, VOL_DEPTH = 6",
                    "PILLAR_X = 2.0f, PILLAR_Y = 0.0f, PILLAR_REACH = 1.5f", "volume_coeff = 200.0f", "crash_threshold = 0.6f"):
        assert literal in txt, literal
    v = pillar_volume()
    assert v.shape == (6, 12, 16) and v.max() > 0.6 and (v == 0).any()
    # the forwarding header is five lines of paths, like its siblings
    fwd = open(os.path.join(REPO, "include", "mppi", "utils", "texture_helpers", "three_d_texture_helper.cuh")).read().splitlines()
    assert len(fwd) == 5 and fwd[3] == '#include "mppi_amd/utils/texture_helpers/three_d_texture_helper.hpp"'


@pytest.mark.gpu
def test_example_runs_and_matches_the_registered_model(gpu, exe):
    """the example's first control sequence (in-kernel Philox noise, seed 42) against a handle on "quadrotor_volume" with the same
    volume, parameters and seed on the templated controller's default form, the fused kernel on (64, 1, 1): equal bit for bit.  Then
    the flight: the vehicle moves towards the goal and keeps clear of the pillar's axis."""
    r = subprocess.run([exe, str(STEPS)], capture_output=True, text=True, timeout=120)
    print(r.stdout[-600:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = re.findall(r"^u\[(\d+)\] = (\S+) (\S+) (\S+) (\S+)$", r.stdout, flags=re.M)
    assert [int(row[0]) for row in rows] == list(range(T)), rows
    first = np.array([[float(v) for v in row[1:]] for row in rows], np.float32)
    end = re.search(r"after (\d+) steps at (\S+) (\S+) (\S+), closest approach to the pillar (\S+) m", r.stdout)
    assert end and int(end.group(1)) == STEPS, r.stdout[-400:]
    assert float(end.group(2)) > 0.3 and float(end.group(5)) > 0.5, end.group(0)

    t3.load_model(m)
    eng = m.VanillaMPPIController("quadrotor_volume", K, T, DT, LAMBDA, 0.0, 1, seed=42, block_x=64, block_y=1,
                                  kernel_variant=m.MPPI_KERNEL_FUSED)
    try:
        eng.setDynamicsParams(m.QuadrotorDynamicsParams())
        eng.setCostParams(example_cost_params())
        m.set_cost_volume(eng, pillar_volume(), origin=(-2.0, -3.0, 0.0), resolution=(CELL, CELL, CELL))
        eng.setSamplingParams([0.5, 0.5, 0.5, 2.0], [1.0] * 4, 0.01, 1.0)
        u0 = np.zeros((T, 4), np.float32)
        u0[:, 3] = 9.81
        eng.updateImportanceSampler(u0)
        x0 = np.zeros(13, np.float32)
        x0[0:3], x0[6] = (0.0, 0.1, 1.5), 1.0
        eng.computeControl(x0, 1)
        info = eng.getLaunchInfo()
        assert info["family"] == "fused" and info["block"] == (64, 1, 1), info
        du = float(np.abs(eng.getControlSeq() - first).max())
        print("u* %.3g from the registered model's" % du)
        assert bits_equal(eng.getControlSeq(), first), du
    finally:
        eng.close()
