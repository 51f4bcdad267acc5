"""evaluateControls / warmStart of the C++ host classes (controllers.hpp and controllers_templated.hpp): one probe program built
with hipcc on Cartpole; what either class returns equals the C ABI's answer on the same handle bit for bit, and the sequence a
warm start installs is the candidate the choice rule of engine/evaluate_host.hpp names."""
import subprocess

import pytest

import mppi_generic_amd as m
import native_build as nb


@pytest.mark.gpu
def test_cpp_host_classes_equal_the_c_abi(gpu):
    exe = nb.build_probe_program(m, "evaluate_controls_cpp.hip")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "evaluate controls cpp ok" in r.stdout and "templated chosen" in r.stdout and "named chosen" in r.stdout
