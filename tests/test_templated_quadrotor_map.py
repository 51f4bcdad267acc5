"""examples/templated_quadrotor_map.hip: the templated Vanilla controller over QuadrotorDynamics + QuadrotorMapCost flies a course
of three gates over a synthetic track map, moving the waypoint with updateWaypoint + setParams between computeControl calls.
The same course, with the example's literal parameters, is flown on the CPU restatement first (tests/quadrotor_map_oracle)."""
import os
import re
import subprocess

import numpy as np
import pytest

import mppi_generic_amd as m
import native_build as nb
import pyoracle as po
import quadrotor_map_oracle as qm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "templated_quadrotor_map"

# the example's literals
K, T, DT, LAMBDA = 256, 40, 0.02, 5.0
GATES = [(3.0, 0.0, 1.2, np.pi / 2), (6.0, 2.0, 1.5, np.pi / 2), (9.0, 2.0, 1.0, np.pi / 2)]
# The CPU restatement, Philox seed 42, passes the three gates after 89, 180 and 265 steps of its closed loop.  Ten seeds need between
# 263 and 284 steps at K = 256, T = 40, and all ten pass.  With gate_margin = 0.5 two of six seeds miss the third gate at this size
# (by 3 and 9 cm) and none of six passes all three at K = 128, T = 30: the course was made easier (margin 0.75 m), not the factor wider.
RESTATEMENT_STEPS = 265
ENGINE_STEPS = int(1.5 * RESTATEMENT_STEPS)  # the engine draws its own Philox noise: 1.5 is the headroom for that


def course_map():
    """distance [m] to the centre line (0, 0) -> (3, 0) -> (6, 2) -> (9, 2); 0.5 m cells over x in [-2, 11), y in [-3, 5)"""
    pts = np.array([[0, 0], [3, 0], [6, 2], [9, 2]], np.float64)
    X, Y = np.meshgrid(-2 + 0.5 * (np.arange(26) + 0.5), -3 + 0.5 * (np.arange(16) + 0.5))
    d = np.full(X.shape, np.inf)
    for a, b in zip(pts[:-1], pts[1:]):
        ab = b - a
        t = np.clip(((X - a[0]) * ab[0] + (Y - a[1]) * ab[1]) / (ab @ ab), 0, 1)
        d = np.minimum(d, np.hypot(X - a[0] - t * ab[0], Y - a[1] - t * ab[1]))
    return d.astype(np.float32), qm.frame15([-2, -3, 0], np.eye(3), [0.5, 0.5, 1.0])


def course_params():
    p = m.QuadrotorMapCostParams()
    p.gate_width, p.gate_margin, p.desired_speed = 1.0, 0.75, 2.0
    p.height_coeff, p.speed_coeff, p.heading_coeff = 50, 20, 50
    p.update_waypoint(0, 0, 1.0, np.pi / 2)
    p.update_waypoint(*GATES[0])
    return p


def test_course_on_the_restatement():
    """the closed loop of the example on the CPU restatement: all three gates, in RESTATEMENT_STEPS steps"""
    p = course_params()
    o = qm.QuadrotorMapOracle(K, T, 1, DT, LAMBDA, 0.0, 1)
    o.set_dynamics_params(m.QuadrotorDynamicsParams())
    o.set_cost_params(p)
    o.set_costmap(*course_map())
    o.set_sampler([0.5, 0.5, 0.5, 2.0], [1.0] * 4)
    u0 = np.zeros((T, 4), np.float32)
    u0[:, 3] = 9.81
    o.set_nominal_control(u0)
    x = np.zeros(13, np.float32)
    x[2], x[6] = 1.0, 1.0
    passed = []
    for i in range(ENGINE_STEPS):
        o.vanilla_compute_control(x, 1, po.philox_normal(42, i, K, T, 4)[None])
        x = o.model_step(x, o.control()[0].copy())[0]
        o.vanilla_slide(1)
        if o.terms(x)[7] < p.gate_margin:
            passed.append(i + 1)
            if len(passed) == 3:
                break
            assert p.update_waypoint(*GATES[len(passed)])
            o.set_cost_params(p)
    print("gates passed after", passed, "steps")
    assert len(passed) == 3 and passed[-1] == RESTATEMENT_STEPS, passed


@pytest.fixture(scope="module")
def exe(lib):
    return nb.build_example(m, NAME)


def test_example_uses_the_reference_spellings_and_builds(exe):
    txt = open(os.path.join(REPO, "examples", NAME + ".hip")).read()
    incs = re.findall(r'#include [<"]([^>"]+)[>"]', txt)
    assert all(i.startswith("mppi/") or "/" not in i for i in incs), incs
    assert "mppi_amd" not in re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert os.access(exe, os.X_OK)
    # the literals of this file are the example's
    for literal in ("HORIZON = 40", "ROLLOUTS = 256", "dt = 0.02f, lambda = 5.0f, alpha = 0.0f", "gate_margin = 0.75f",
                    "{ 3.0f, 0.0f, 1.2f, half_pi }, { 6.0f, 2.0f, 1.5f, half_pi }, { 9.0f, 2.0f, 1.0f, half_pi }"):
        assert literal in txt, literal


@pytest.mark.gpu
def test_engine_flies_the_course(gpu, exe):
    """the example on the engine, with its own in-kernel Philox noise: all three gates within 1.5 x the restatement's step count"""
    r = subprocess.run([exe, str(ENGINE_STEPS)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    passed = [int(s) for s in re.findall(r"gate \d passed at step (\d+)", r.stdout)]
    assert len(passed) == 3 and passed == sorted(passed) and passed[-1] <= ENGINE_STEPS, passed
    assert "3 of 3 gates passed" in r.stdout
