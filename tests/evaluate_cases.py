"""What the tests of mppi_evaluate_controls / mppi_warm_start share: the pure-Python reference of the warm-start choice and the
oracle's trajectory cost and last crash status of caller-supplied control rows.  Checked on the CPU (tests/test_evaluate_host.py)
before the GPU tests (tests/test_evaluate_gpu.py) rely on them."""
import copy

import numpy as np

from common import make_oracle
from replay_cases import oracle_row, selection_reference

F = np.float32


def choice_reference(costs, hysteresis):
    """costs (n + 1,): the current sequence's cost, then the candidates'.  The winner of all n + 1 in mppi_top_rollouts' order
    (ascending, ties to the lower index — the current sequence is index 0 —, NaN last); a winning candidate is installed only
    if its cost is below current - hysteresis in float32, or if the current cost is NaN (the winner's then is not).  Returns
    the candidate's index, or -1: the current sequence stays."""
    costs = np.asarray(costs, np.float32)
    w = int(selection_reference(costs, 1)[0][0])
    if w == 0:
        return -1
    if np.isnan(costs[0]):
        return w - 1
    return w - 1 if costs[w] < F(costs[0] - F(hysteresis)) else -1


def oracle_twin(cfg, n):
    """the oracle of cfg with K = n rollouts and no control cost: its likelihood-ratio term is exactly zero"""
    twin = copy.copy(cfg)
    twin["K"] = int(n)
    twin["D"] = 1
    twin["control_cost_coeff"] = [0.0] * len(cfg["std_dev"])
    return make_oracle(twin), twin


def oracle_costs(orc, twin, x0, u):
    """(costs (n,), clamped rows (n, T, C)) of the rows u (n, T, C) from x0 (S,): Oracle.rollout_costs with the rows as v"""
    n, T, C = u.shape
    costs, v = orc.rollout_costs(x0, np.zeros((1, T, C), np.float32), u.reshape(1, n, T, C))
    return costs[0], v[0]


def oracle_last_crash(orc, twin, x0, v_rows):
    """the crash status after the last step of already clamped rows (a model without a control deadband: constraining such a
    row again is the identity)"""
    return np.array([oracle_row(orc, twin, x0, row)[2][-1] for row in v_rows], np.int32)
