"""Replay of sampled rollouts, the parts that need no device: the float32 restatement of how step costs fold into a trajectory
cost (held to the oracle's rollout_costs bit for bit — the GPU tests reuse it), the reference of the selection order, the exported
symbols, and the host-side refusals and list builder."""
import os
import re
import subprocess

import numpy as np
import pytest

import mppi_generic_amd as m
import native_build as nb
from common import cartpole_cfg_lr, di_cfg, host_noise, make_oracle, ulp_diff
from replay_cases import boundary_rows, fold_step_costs, oracle_row, selection_reference

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lr_cfg(name):
    if name == "cartpole":
        return cartpole_cfg_lr(K=65, T=9)
    cfg = di_cfg(K=130, T=17, tube=False)
    cfg["control_cost_coeff"] = [0.3, 0.2]
    cfg["alpha"] = 0.1
    cfg["ranges"] = [[-3.0, 3.0], [-3.0, 3.0]]
    return cfg


def cartpole_terminal(cfg, orc):
    """CartpoleQuadraticCost::terminalCost = the state cost times terminal_cost_coeff"""
    coeff = np.float32(cfg["cost"].terminal_cost_coeff)
    return lambda y: np.float32(np.float32(orc.state_cost(y, 0, 0)[0]) * coeff)


@pytest.mark.parametrize("name", ["cartpole", "double_integrator"])
def test_step_cost_fold_equals_the_oracle_trajectory_cost(name):
    cfg = _lr_cfg(name)
    orc = make_oracle(cfg)
    K, T, C = cfg["K"], cfg["T"], len(cfg["std_dev"])
    mean = (0.4 * np.sin(np.arange(T * C, dtype=np.float32))).reshape(1, T, C).astype(np.float32)
    v = orc.set_gaussian_controls(mean, host_noise(1, K, T, C)[0])
    costs, v = orc.rollout_costs(cfg["x0"], mean, v)
    terminal = cartpole_terminal(cfg, orc) if name == "cartpole" else None
    rows = boundary_rows(K)
    steps = np.stack([oracle_row(orc, cfg, cfg["x0"], v[0, k], mean[0], int(k), terminal)[1] for k in rows])
    assert np.abs(steps[:, :T]).max() > 0 and (name != "cartpole" or np.abs(steps[:, T]).max() > 0)
    assert int(ulp_diff(fold_step_costs(steps), costs[0, rows]).max()) == 0


def test_selection_reference_order():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    costs = np.array([3, 1, nan, 1, -inf, inf, 0.0, -0.0, 2, inf, nan, 1], np.float32)
    idx, val = selection_reference(costs, costs.size)
    assert idx.tolist() == [4, 6, 7, 1, 3, 11, 8, 0, 5, 9, 2, 10]  # ties (1, 1, 1; 0.0, -0.0; inf, inf) by index, NaN last
    assert np.isnan(val[-2:]).all() and not np.isnan(val[:-2]).any()
    idx3, val3 = selection_reference(costs, 3)
    assert idx3.tolist() == [4, 6, 7] and val3.tolist() == [-inf, 0.0, -0.0]


def test_declared_replay_symbols_are_exported_and_bound(lib):
    txt = open(os.path.join(REPO, "include", "mppi_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("mppi_top_rollouts", "mppi_replay_rollouts"):
        assert re.search(r"\b%s\s*\(" % name, txt), name + " is not declared in include/mppi_amd.h"
        assert hasattr(lib, name), "libmppi_amd.so does not export " + name
        assert name in m.SIGNATURES


def test_null_handle_is_refused(lib):
    idx = np.zeros(1, np.int32)
    assert lib.mppi_top_rollouts(None, 0, 1, idx.ctypes.data, None) == m.MPPI_ERR_INVALID_ARG
    assert lib.mppi_replay_rollouts(None, 0, idx.ctypes.data, 1, None, None, None) == m.MPPI_ERR_INVALID_ARG


def test_sampled_trajectory_list():
    lst = m.sampled_trajectory_list(1049, 0.0)
    assert lst.tolist() == [-1]
    lst = m.sampled_trajectory_list(1049, 0.05, seed=3)
    assert lst[0] == -1 and lst.size == 1 + int(0.05 * 1049)
    body = lst[1:]
    assert len(set(body.tolist())) == body.size and body.min() >= 0 and body.max() < int(1049 * 0.98)
    assert np.array_equal(lst, m.sampled_trajectory_list(1049, 0.05, seed=3))
    assert not np.array_equal(lst, m.sampled_trajectory_list(1049, 0.05, seed=4))
    assert m.sampled_trajectory_list(200, 0.99).tolist() == [-1] + list(range(198))  # above 0.98: 0, 1, 2, ...


def test_host_checks_under_the_sanitizers(tmp_path):
    """the index validation and the C++ list builder (include/mppi_amd/engine/replay_host.hpp) in a stand-alone program built
    with the address and undefined-behaviour sanitizers"""
    src = os.path.join(REPO, "tests", "probes", "replay_host_probe.cpp")
    exe = nb.build(tmp_path / "replay_host_probe", [nb.cxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                                                     "-fno-sanitize-recover=all", "-I" + nb.INCLUDE, src], [src], "replay_host_probe")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "replay host checks ok" in r.stdout
