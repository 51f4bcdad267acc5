"""The DDP backward pass of include/mppi_amd/feedback_controllers/ddp_backward.hpp, built for the host (tests/feedback_host),
against float64 (CPU; the device side is tests/test_feedback_gpu.py).

The reference is this file's own text: ddp/ddp.h:77-127 of MPPI-Generic with DDPFeedback's costs in numpy float64 (`ddp_f64`), fed
the SAME float32 A, B the host build gets — the shipped computeGrad of each model (tests/linearize_host) at the points of
tests/linearize_cases.py, cycled into sequences of T = 2, 3 and 50, dt = 0.02.  Weights: identities (the DDPParams default) for
every model, and Q = diag(500, 500, 100, 100), R = I, Qf = I for the double integrator.

Yardstick: per time step, the largest |L_host - L_f64| over the entries of L_t divided by the largest |L_t| (float64); the worst
over the steps and cases of a model.  Measured with this file (test_host_build_against_float64 prints them):

    model               worst |dL| / max|L_t|    bound (2 x)
    cartpole            4.30e-07                 8.60e-07
    double_integrator   3.06e-07                 6.12e-07
    racer_dubins        6.01e-07                 1.20e-06
    quadrotor           7.65e-07                 1.53e-06

The factor 2 is for the device build of the same header, which gives the same bits (test_feedback_gpu.py) — not for new error.
Every bound is far below 1e-3, above which a comparison would say nothing about the recursion.  In float64 every unpivoted pivot
of quu of every case is > 0 (asserted): the unpivoted LDL^T the header uses is defined wherever these tests go.
"""
import numpy as np
import pytest

import feedback_host as fh
import linearize_cases as lc
import linearize_host as lh

DT = 0.02
HORIZONS = (2, 3, 50)
MODELS = ("cartpole", "double_integrator", "racer_dubins", "quadrotor")
HOST_PARAMS = {"cartpole": lc.CARTPOLE_PARAMS[1], "quadrotor": lc.QUADROTOR_PARAMS[1]}
# twice the measured worst relative deviation (module docstring)
BOUND = {"cartpole": 2 * 4.30e-07, "double_integrator": 2 * 3.06e-07, "racer_dubins": 2 * 6.01e-07, "quadrotor": 2 * 7.65e-07}
ACCEPTANCE_Q = np.diag([500.0, 500.0, 100.0, 100.0])


def unpivoted_pivots(M):
    """the pivots d of M = L D L^T without pivoting, float64"""
    n = M.shape[0]
    L, d = np.eye(n), np.zeros(n)
    for j in range(n):
        d[j] = M[j, j] - (L[j, :j] ** 2 * d[:j]).sum()
        for i in range(j + 1, n):
            L[i, j] = (M[i, j] - (L[i, :j] * L[j, :j] * d[:j]).sum()) / d[j]
    return d


def ddp_f64(A, B, Q, R, Qf, dt):
    """ddp.h:77-127 in float64: (L [T][C][S], the smallest unpivoted pivot of any quu)"""
    A, B = A.astype(np.float64), B.astype(np.float64)
    T, S, C = B.shape
    Q, R, Qf = (np.asarray(M, np.float64) for M in (Q, R, Qf))
    L = np.zeros((T, C, S))
    Vxx = 0.5 * (Qf + Qf.T)
    least = np.inf
    for k in range(T - 2, -1, -1):
        Phi, Bd = A[k] * dt + np.eye(S), B[k] * dt
        qux = Bd.T @ Vxx @ Phi
        qxx = Q * dt + Phi.T @ Vxx @ Phi
        quu = R * dt + Bd.T @ Vxx @ Bd
        least = min(least, unpivoted_pivots(quu).min())
        L[k] = np.linalg.solve(quu, -qux)
        Vxx = qxx + qux.T @ L[k]
        Vxx = 0.5 * (Vxx + Vxx.T)
    return L, least


def jacobians(model, T):
    """float32 A (T, S, S), B (T, S, C) of the shipped class at the model's test points, cycled"""
    xs, us = lc.POINTS[model]()
    idx = np.arange(T) % xs.shape[0]
    kw = dict(params=HOST_PARAMS[model]) if model in HOST_PARAMS else {}
    A, B, _ = lh.host_grad(model, xs[idx], us[idx], **kw)
    return A, B


def weight_sets(model):
    S, C = lh.DIMS[model]
    sets = [(np.eye(S), np.eye(C), np.eye(S))]
    if model == "double_integrator":
        sets.append((ACCEPTANCE_Q, np.eye(C), np.eye(S)))
    return sets


def relative_deviation(G_host, L64):
    """worst over the steps of max|dL_t| / max|L_t|; G is [T][S][C] with G[t][i][j] = L_t[j][i]"""
    L_host = G_host.transpose(0, 2, 1).astype(np.float64)
    worst = 0.0
    for t in range(L64.shape[0]):
        scale = np.abs(L64[t]).max()
        if scale > 0:
            worst = max(worst, np.abs(L_host[t] - L64[t]).max() / scale)
        else:
            assert not L_host[t].any()
    return worst


@pytest.mark.parametrize("model", MODELS)
def test_host_build_against_float64(model):
    worst = 0.0
    for T in HORIZONS:
        A, B = jacobians(model, T)
        for Q, R, Qf in weight_sets(model):
            L64, least_pivot = ddp_f64(A, B, Q, R, Qf, DT)
            assert least_pivot > 0, (model, T, least_pivot)  # the condition the unpivoted factorisation needs, no case dropped
            G, ok, step = fh.host_gains(A, B, DT, Q, R, Qf)
            assert ok and step == -1 and np.isfinite(G).all()
            assert not G[T - 1].any()  # the reference's Lk_ at H - 1: zero-initialised, never written
            if T == 50:
                assert np.abs(G[:T - 1]).max() > 0
            worst = max(worst, relative_deviation(G, L64))
    print("%-18s worst |dL| / max|L_t| = %.3g (bound %.3g)" % (model, worst, BOUND[model]))
    assert BOUND[model] < 1e-3
    assert worst <= BOUND[model], (model, worst, BOUND[model])


def test_double_integrator_at_the_acceptance_size():
    """T = 50, dt = 0.02, Q = diag(500, 500, 100, 100), R = I, Qf = I: the textbook LQR recursion with np.linalg.solve"""
    T = 50
    A, B = jacobians("double_integrator", T)
    Phi, Bd = np.eye(4) + A[0].astype(np.float64) * DT, B[0].astype(np.float64) * DT
    Qd, Rd = ACCEPTANCE_Q * DT, np.eye(2) * DT
    P = np.eye(4)
    L = np.zeros((T, 2, 4))
    for k in range(T - 2, -1, -1):
        L[k] = -np.linalg.solve(Rd + Bd.T @ P @ Bd, Bd.T @ P @ Phi)
        P = Qd + Phi.T @ P @ Phi + (Bd.T @ P @ Phi).T @ L[k]
        P = 0.5 * (P + P.T)
    G, ok, step = fh.host_gains(A, B, DT, ACCEPTANCE_Q, np.eye(2), np.eye(4))
    assert ok and step == -1
    assert G.shape == (T, 4, 2) and not G[T - 1].any()
    assert relative_deviation(G, L) <= BOUND["double_integrator"]
    # the layout: G[t][i][j] = L_t[j][i], the position gains of control 0 on state 0 and of control 1 on state 1
    for t in (0, 17, T - 2):
        for i in range(4):
            for j in range(2):
                assert abs(G[t, i, j] - L[t, j, i]) <= BOUND["double_integrator"] * np.abs(L[t]).max()
    assert G[0, 0, 0] < -1 and G[0, 1, 1] < -1 and G[0, 0, 1] == 0 and G[0, 1, 0] == 0


def test_failed_pivot_stops_at_the_first_step_and_writes_nothing():
    """R = 0 and a B whose columns are zero: quu = 0 at the first step of the pass, k = T - 2"""
    T = 6
    A, B = jacobians("double_integrator", T)
    B = np.zeros_like(B)
    out = np.full((T, 4, 2), -3.0, np.float32)
    G, ok, step = fh.host_gains(A, B, DT, R=np.zeros((2, 2)), out=out)
    assert not ok and step == T - 2
    assert (out == -3.0).all()
    # a NaN in the Jacobians of step 2 reaches Vxx there and is a failed pivot of the step below it; the rows from the failing
    # step down and row T - 1 are untouched
    A, B = jacobians("double_integrator", T)
    A[2, 0, 0] = np.nan
    G, ok, step = fh.host_gains(A, B, DT, out=out)
    assert not ok and step == 1
    assert (out[:2] == -3.0).all() and (out[T - 1] == -3.0).all() and np.isfinite(out[3:T - 1]).all()


def test_terminal_weight_is_symmetrised():
    T = 5
    A, B = jacobians("cartpole", T)
    rng = np.random.default_rng(3)
    M = rng.uniform(-0.2, 0.2, (4, 4)).astype(np.float32)
    Qf = (np.eye(4, dtype=np.float32) * 2 + M).astype(np.float32)
    sym = (np.float32(0.5) * (Qf + Qf.T)).astype(np.float32)
    assert (Qf != Qf.T).any()
    G, ok, _ = fh.host_gains(A, B, DT, Qf=Qf)
    G_sym, ok_sym, _ = fh.host_gains(A, B, DT, Qf=sym)
    assert ok and ok_sym
    assert (G.view(np.uint32) == G_sym.view(np.uint32)).all()
    G_t, _, _ = fh.host_gains(A, B, DT, Qf=np.ascontiguousarray(Qf.T))
    assert (G.view(np.uint32) == G_t.view(np.uint32)).all()
    L64, _ = ddp_f64(A, B, np.eye(4), np.eye(1), Qf, DT)
    assert relative_deviation(G, L64) <= BOUND["cartpole"]
