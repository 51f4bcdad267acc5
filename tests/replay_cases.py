"""What the replay tests share: the numpy restatement of how step costs fold into a trajectory cost, the pure-Python reference of
the selection order, and the oracle's per-step quantities of one control row.  Checked on the CPU (tests/test_replay_host.py)
before the GPU tests (tests/test_replay_gpu.py) rely on them."""
import math

import numpy as np

F = np.float32


def fold_step_costs(step_costs):
    """step_costs (n, T + 1) -> trajectory costs (n,), in the order of the rollout kernel and of the oracle
    (oracle/oracle_core.hpp rolloutCosts): a serial float32 sum over t, then running / T + terminal / T"""
    c = np.ascontiguousarray(step_costs, np.float32)
    n, T = c.shape[0], c.shape[1] - 1
    out = np.empty(n, np.float32)
    for r in range(n):
        running = F(0.0)
        for t in range(T):
            running = F(running + c[r, t])
        out[r] = F(F(running / F(T)) + F(c[r, T] / F(T)))
    return out


def selection_reference(costs, n):
    """the n lowest costs: ascending, ties to the lower index, NaN after every number (+inf included)"""
    costs = np.asarray(costs, np.float32)
    order = sorted(range(costs.size), key=lambda i: (1, 0.0, i) if math.isnan(costs[i]) else (0, float(costs[i]), i))
    idx = np.array(order[:n], np.int32)
    return idx, costs[idx]


def likelihood_ratio(u, mean_t, std_dev, coeff, lambda_, alpha, pure=False):
    """GaussianSampler::likelihoodRatioCost (oracle/oracle_core.hpp) in float32, operation for operation"""
    C = len(u)
    width = 4 if C % 4 == 0 else (2 if C % 2 == 0 else 1)
    term = lambda j: F(F(F(F(coeff[j]) * m(j)) * F(m(j) - F(F(2.0) * F(u[j])))) / F(F(std_dev[j]) * F(std_dev[j])))  # noqa: E731
    m = lambda j: F(0.0) if pure else F(mean_t[j])  # noqa: E731
    cost = F(0.0)
    if width > 1:
        lane = [F(0.0)] * 4
        for i in range(C // width):
            for l in range(width):
                lane[l] = F(lane[l] + term(i * width + l))
        s = F(lane[0] + lane[1])
        if width == 4:
            s = F(F(s + lane[2]) + lane[3])
        cost = F(cost + s)
    else:
        for j in range(C):
            cost = F(cost + term(j))
    return F(F(F(F(0.5) * F(lambda_)) * F(F(1.0) - F(alpha))) * cost)


def oracle_row(orc, cfg, x0, u_row, mean=None, k=0, terminal=None):
    """one control row through the oracle: outputs after each step (T, O), step costs (T + 1,), crash flags (T,).
    mean: the control mean [T][C] of the likelihood-ratio term (None: the term is zero, control_cost_coeff == 0);
    terminal(y) -> the terminal cost of the last output (None: 0)"""
    T = cfg["T"]
    u_row = np.ascontiguousarray(u_row, np.float32)
    xs, ys = orc.output_trajectory(x0, u_row)
    _, _, y_last = orc.model_step_full(xs[T - 1], u_row[T - 1])
    y = np.concatenate([ys[1:], y_last[None, :]], axis=0)
    cost = np.zeros(T + 1, np.float32)
    crash = np.zeros(T, np.int32)
    cr = 0
    pure = bool(F(k) >= F(F(F(1.0) - F(cfg.get("pure_pct", 0.01))) * F(cfg["K"])))  # gaussian.cu:108, in float
    for t in range(T):
        c, cr = orc.state_cost(y[t], t, cr)
        lr = F(0.0)
        if mean is not None:
            lr = likelihood_ratio(u_row[t], mean[t], cfg["std_dev"], cfg["control_cost_coeff"], cfg["lambda_"], cfg["alpha"], pure)
        cost[t] = F(F(c) + lr)
        crash[t] = cr
    cost[T] = F(0.0) if terminal is None else F(terminal(y[T - 1]))
    return y, cost, crash


def boundary_rows(K, pure_pct=0.01):
    """nine rows: the first and the last rollout, the rows around the pure-noise boundary and around a wave boundary"""
    pure0 = int(math.ceil((1.0 - pure_pct) * K))
    rows = [0, 1, 63 % K, 64 % K, 65 % K, max(pure0 - 1, 0), min(pure0, K - 1), K - 2, K - 1]
    out = []
    for r in rows:
        r = min(max(r, 0), K - 1)
        while r in out:
            r = (r + 7) % K
        out.append(r)
    return np.array(out, np.int32)
