"""The reference-named sampled-trajectory methods of the templated C++ host classes (setTopNSampledControlTrajectories,
setPercentageSampledControlTrajectories, calculateSampledStateTrajectories, getSampled*Trajectories, getTopNCosts): one probe
program built with hipcc on Cartpole; its first top-N index and cost equal the C ABI's and a scan of all costs."""
import os
import re
import subprocess

import pytest

import mppi_generic_amd as m
import native_build as nb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_templated_sampled_trajectories_equal_the_c_abi(gpu, tmp_path):
    src = os.path.join(REPO, "tests", "probes", "sampled_trajectories_templated.hip")
    exe = nb.build(tmp_path / "sampled_trajectories_templated", nb.hip_exe(m, src), [src], "sampled_trajectories_templated")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    mt = re.search(r"class (-?\d+) (\S+) abi (-?\d+) (\S+) scan (-?\d+) (\S+)", r.stdout)
    assert mt, r.stdout[-500:]
    assert mt.group(1) == mt.group(3) == mt.group(5), r.stdout
    assert mt.group(2) == mt.group(4) == mt.group(6), r.stdout
    assert "shapes 1 1 1" in r.stdout
