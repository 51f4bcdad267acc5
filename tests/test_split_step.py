"""The split Cartpole step (plugin/dynamics.hpp: SPLIT_STEP_CLASS, stepCore / stepComplete) on rolloutPipelineKernel: the
dynamics wave advances (theta, theta_dot) and rings a carry, the cost wave rebuilds the cart's states from it.

  CPU  the capability binds to the most-derived class only (a subclass of CartpoleDynamics runs step())
  CPU  the headline instantiation's dynamics-wave loop stays at or below the instruction count the split brought it to
  GPU  at bench.py's size, Philox and injected noise: trajectory costs 0 ulp, u* within 1e-5 of the oracle, and the launch is
       the one-system pipeline — the streamed-merge form on later iterations
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import native_build as nb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what the split leaves on the headline kernel's dynamics wave (tools/isa_step_count.py; 89.62 before it)
DYN_WAVE_MAX_INSTRUCTIONS_PER_STEP = 74.38

TRAIT_TU = r"""
#include "mppi_amd/dynamics/cartpole/cartpole_dynamics.hpp"
#include "mppi_amd/engine/rollout_pipeline_kernel.hpp"

class MyCartpole : public CartpoleDynamics
{
public:
  __device__ inline void computeDynamics(float* state, float* control, float* state_der, float* theta = nullptr)
  {
    CartpoleDynamics::computeDynamics(state, control, state_der, theta);
    state_der[3] *= 0.5f;
  }
};

static_assert(mppi::split_step<CartpoleDynamics>::value, "CartpoleDynamics declares the split step");
static_assert(!mppi::split_step<MyCartpole>::value, "a class derived from a split plugin must fall back to step()");
static_assert(mppi::kernels::pipeRingOutputFloats<CartpoleDynamics>() == CartpoleDynamics::SPLIT_CARRY, "ring carries the carry");
static_assert(mppi::kernels::pipeRingOutputFloats<MyCartpole>() == MyCartpole::OUTPUT_DIM, "ring carries the output");
int main() { return 0; }
"""


def test_split_capability_binds_to_the_most_derived_class(tmp_path):
    src = tmp_path / "split_trait.hip"
    src.write_text(TRAIT_TU)
    r = nb.hip_syntax_only(src)
    assert r.returncode == 0, r.stderr[-4000:]


def test_headline_dynamics_wave_instruction_count():
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "isa_step_count.py")], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout)
    dyn, cost = got["cartpole_pipeline_dynamics_wave"], got["cartpole_pipeline_cost_wave"]
    assert dyn["steps_per_trip"] == 8 and cost["steps_per_trip"] == 4, (dyn, cost)
    assert dyn["instructions_per_step"] <= DYN_WAVE_MAX_INSTRUCTIONS_PER_STEP, dyn
    # the two entries are two different loops (the tool tells them apart by who stores and who reads the ring)
    assert dyn["loop_instructions"] != cost["loop_instructions"]


def _run(noise, num_iters):
    import pyoracle as po
    from common import cartpole_cfg, host_noise, make_engine, make_oracle, ulp_diff
    cfg = cartpole_cfg(K=16384, T=100, soft=True, num_iters=num_iters)
    eng, orc = make_engine(cfg), make_oracle(cfg)
    if noise == "injected":
        eps = host_noise(num_iters, cfg["K"], cfg["T"], 1)
        eng.injectNoise(eps)
    else:
        eng.setSeed(42)
        eps = np.stack([po.philox_normal(42, g, cfg["K"], cfg["T"], 1) for g in range(num_iters)])
    eng.computeControl(cfg["x0"], 1)
    orc.vanilla_compute_control(cfg["x0"], 1, eps)
    info = eng.getLaunchInfo()
    du = float(np.abs(eng.getControlSeq() - orc.control()).max())
    costs = (eng.getSampledCostSeq(), orc.costs())
    eng.close()
    return info, du, costs, ulp_diff


@pytest.mark.gpu
@pytest.mark.parametrize("noise", ["philox", "injected"])
def test_split_step_pipeline_at_bench_size_vs_oracle(gpu, noise):
    info, du, (ce, co), ulp_diff = _run(noise, 1)
    assert info == dict(family="pipeline", block=(64, 1, 1), rows_in_hbm=False, streamed_merge=False), info
    dc = int(ulp_diff(ce, co).max())
    assert dc == 0, "trajectory costs differ from the oracle by %d ulp" % dc
    assert du <= 1e-5, du


@pytest.mark.gpu
def test_split_step_headline_kernel_vs_oracle(gpu):
    """bench.py's kernel: the streamed-merge instantiation, from the second iteration of a Philox handle on"""
    info, du, (ce, co), _ = _run("philox", 3)
    assert info == dict(family="pipeline", block=(64, 1, 1), rows_in_hbm=False, streamed_merge=True), info
    # after the first iteration the mean carries the ~1e-7 difference of the first u* (test_full_size_parity.py)
    np.testing.assert_allclose(ce, co, rtol=1e-5)
    assert du <= 1e-5, du
