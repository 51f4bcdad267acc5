"""mppi_evaluate_controls and mppi_warm_start on the device.

The reference of every cost is pyoracle.Oracle.rollout_costs on an oracle twin with control_cost_coeff = 0 (its likelihood-ratio
term is then exactly zero), K = n and the caller's rows as v, once per distinct start state; costs at 0 ulp, crash flags equal.
Shapes: n in {1, rows - 1, rows, rows + 1, 2 rows + 3} with `rows` the rows per block of the lane form the model evaluates on
(64 one lane per row; 16 AutoRally's replicated lanes; 1 its one-rollout-per-wave form and the two-lane contract form), T in
{1, 3, 9}, and 17 on the replicated lanes.  The two-lane (BY > 1) case is the LSTM-steering RACER model with a network of another
shape than its four-lane form is compiled for: its finalize form is the model itself on FIN_BY = 2 lanes, and it has an oracle
(the reference-style pendulum plugin of tests/test_plugin_model.py is registered with FIN_BY = 1 and has none; it is held to
the rollout kernel's own costs instead).

From AutoRally's off-track start every row has crashed by its third step and none after its first, whatever the controls, so the
sticky-crash case mixes that start and the on-track one over the rows (x0_count = n).

Measured on an MI355X: every comparison below at 0 ulp."""
import ctypes as C
import gc
import os

import numpy as np
import pytest

import mppi_generic_amd as m
import native_build as nb
from common import SEED, autorally_cfg, cartpole_cfg, di_cfg, host_noise, make_engine, make_pair, racer_cfg, rm_cfg, ulp_diff
from evaluate_cases import choice_reference, oracle_costs, oracle_last_crash, oracle_twin
from kernel_forms import env_override
from racer_cfgs import steering_cfg
from replay_cases import fold_step_costs

pytestmark = pytest.mark.gpu

AR_OFF_TRACK = np.array([-12.0, 4.85, 1.57, 0.0, 8.0, 0.0, 0.0], np.float32)  # the start tests/test_replay_gpu.py uses
ROBUST_TEXT = ("mppi_warm_start: the nominal system of a Robust MPPI handle is chosen by its candidate-state search; installing a "
               "control sequence under it is not supported")


def two_lane_cfg(T):
    """LSTM steering with H = 6 and an output network {10, 12, 1}: the four-lane form refuses it, the finalize form is FIN_BY = 2"""
    rng = np.random.default_rng(2)
    cfg = steering_cfg(K=64, T=T)
    Hn = 6
    blobs = {"lstm_structure": np.array([Hn, Hn + 4, 12, 1], np.float32),
             "lstm_weights": rng.uniform(-0.4, 0.4, 4 * Hn * Hn + 4 * Hn * 4 + 6 * Hn).astype(np.float32),
             "lstm_output_weights": rng.uniform(-0.4, 0.4, (Hn + 4) * 12 + 12 + 12 + 1).astype(np.float32)}
    maps = {k: v for k, v in cfg["blobs"].items() if k.startswith("elevation")}
    cfg["blobs"] = {**blobs, **maps}  # the structure first, then the weights
    return cfg


# name -> (cfg(T), rows per block, MPPI_AMD_FINALIZE_FORM, amplitude of the drawn controls, horizons)
FORMS = {
    "cartpole": (lambda T: cartpole_cfg(K=64, T=T, soft=True), 64, None, 4.0, (1, 3, 9)),
    "double_integrator": (lambda T: di_cfg(K=64, T=T, tube=False), 64, None, 2.0, (1, 3, 9)),
    "racer_dubins": (lambda T: racer_cfg(K=64, T=T), 64, None, 1.5, (1, 3, 9)),
    "autorally_nn-wave": (lambda T: autorally_cfg(K=64, T=T), 1, None, 1.3, (1, 3, 9)),
    "autorally_nn-rep": (lambda T: autorally_cfg(K=64, T=T), 16, "rep", 1.3, (1, 3, 9, 17)),
    "lstm_steering-two-lanes": (two_lane_cfg, 1, None, 1.5, (1, 3, 9)),
}


def row_counts(rows):
    return sorted({n for n in (1, rows - 1, rows, rows + 1, 2 * rows + 3) if n >= 1})


def draw_rows(name, cfg, n, T, amplitude, seed=3):
    C_ = len(cfg["std_dev"])
    u = np.random.default_rng(seed + 100 * n + T).uniform(-amplitude, amplitude, (n, T, C_)).astype(np.float32)
    if name == "cartpole":  # half the rows leave the control range [-5, 5] above, the other half below
        u[0::2, 0::2] = np.float32(5.5) + np.abs(u[0::2, 0::2])
        u[1::2, 0::2] = np.float32(-5.5) - np.abs(u[1::2, 0::2])
    return u


def check_against_the_oracle(eng, cfg, x0, u, crash_too=True, tag=None):
    n = u.shape[0]
    orc, twin = oracle_twin(cfg, n)
    want, v = oracle_costs(orc, twin, x0, u)
    cost, crash = eng.evaluate_controls(x0, u)
    assert cost.shape == (n,) and crash.shape == (n,)
    assert int(ulp_diff(cost, want).max()) == 0, (tag, cost[:4], want[:4])
    if crash_too:
        assert np.array_equal(crash, oracle_last_crash(orc, twin, x0, v)), tag
    return cost, crash, v


# ------------------------------------------------------------------ 1. every lane form against the oracle ----------------
@pytest.mark.parametrize("name", list(FORMS))
def test_costs_equal_the_oracle_on_every_lane_form(gpu, name):
    make_cfg, rows, form, amplitude, horizons = FORMS[name]
    with env_override(MPPI_AMD_FINALIZE_FORM=form):
        for T in horizons:
            cfg = make_cfg(T)
            eng = make_engine(cfg)  # no iteration runs on it: the call works on a fresh handle
            for n in row_counts(rows):
                u = draw_rows(name, cfg, n, T, amplitude)
                _, _, v = check_against_the_oracle(eng, cfg, cfg["x0"], u, tag=(name, T, n))
                if name == "cartpole":  # the clamp acts in every row, on each side in half of them
                    assert (v[0::2].max(axis=(1, 2)) == 5.0).all() and (u[0::2].max(axis=(1, 2)) > 5.0).all()
                    assert n == 1 or ((v[1::2].min(axis=(1, 2)) == -5.0).all() and (u[1::2].min(axis=(1, 2)) < -5.0).all())
            eng.close()


def test_reference_style_pendulum_plugin_reproduces_the_rollout_kernel(gpu):
    """a user's model with its own __syncthreads() and sinf / cosf, built on its own: no oracle, so the rows the rollout kernel
    saved are evaluated again and must give the costs it gave them (zero control cost coefficient: no likelihood-ratio term)"""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(repo, "examples", "my_model", "pendulum_model_reference_style.hip")
    hdr = [os.path.join(repo, "examples", "my_model", "pendulum_reference_style.cuh")]
    nb.load_plugin_model(m, "user_pendulum_reference_style", src, os.path.join(repo, "examples", "_build",
                                                                                 "libpendulum_model_reference_style.so"), hdr)
    K, T = 130, 9
    eng = m.VanillaMPPIController("user_pendulum_reference_style", K, T, 0.02, 1.0, 0.0, 1, seed=SEED, save_samples=True)
    eng.setDynamicsParams((C.c_float * 4)(1.0, 1.0, 0.1, 9.81))
    eng.setCostParams((C.c_float * 6)(0.0, 1.0, 10.0, 0.1, 0.0, np.pi))
    eng.setControlRanges([[-4.0, 4.0]])
    eng.setSamplingParams([2.0], [0.0])
    eng.injectNoise(host_noise(1, K, T, 1))
    x0 = np.array([0.3, 0.0], np.float32)
    costs = eng.rolloutCosts(x0, 1)[0]
    cost, crash = eng.evaluate_controls(x0, eng.getSampledControls()[0])
    assert int(ulp_diff(cost, costs).max()) == 0 and np.unique(costs).size > K // 2
    assert not crash.any()
    eng.close()


# ------------------------------------------------------------------ 2. one initial state per row -------------------------
@pytest.mark.parametrize("name,n,T", [("cartpole", 131, 9), ("autorally_nn-rep", 35, 3), ("autorally_nn-wave", 5, 3)])
def test_per_row_initial_states(gpu, name, n, T):
    """three distinct states interleaved over the rows against three oracle calls; one state for all rows == n copies of it"""
    make_cfg, _, form, amplitude, _ = FORMS[name]
    cfg = make_cfg(T)
    S = cfg["x0"].size
    states = np.stack([cfg["x0"], cfg["x0"] + np.float32(0.125), cfg["x0"] - np.float32(0.0625) * np.arange(S, dtype=np.float32)])
    u = draw_rows(name, cfg, n, T, amplitude)
    orc, twin = oracle_twin(cfg, n)
    per_state = [oracle_costs(orc, twin, s, u) for s in states]
    which = np.arange(n) % 3
    want = np.array([per_state[which[i]][0][i] for i in range(n)], np.float32)
    with env_override(MPPI_AMD_FINALIZE_FORM=form):
        eng = make_engine(cfg)
        cost, crash = eng.evaluate_controls(states[which], u)
        assert int(ulp_diff(cost, want).max()) == 0
        for a, b in ((0, 1), (1, 2), (0, 2)):  # the three states do give three costs, in every row
            assert (per_state[a][0] != per_state[b][0]).all()
        for s in range(3):
            rows = np.flatnonzero(which == s)
            assert np.array_equal(crash[rows], oracle_last_crash(orc, twin, states[s], per_state[s][1][rows]))
        one, one_crash = eng.evaluate_controls(states[1], u)
        copies, copies_crash = eng.evaluate_controls(np.repeat(states[1][None, :], n, axis=0), u)
        assert np.array_equal(one.view(np.int32), copies.view(np.int32)) and np.array_equal(one_crash, copies_crash)
        assert int(ulp_diff(one, per_state[1][0]).max()) == 0
        eng.close()


# ------------------------------------------------------------------ 3. the crash status -----------------------------------
@pytest.mark.parametrize("form", [None, "rep"])
def test_crash_status_after_the_last_step(gpu, form):
    T, n = 9, 35
    cfg = autorally_cfg(K=64, T=T)
    u = draw_rows("autorally_nn", cfg, n, T, 1.3)
    starts = np.where((np.arange(n) % 2 == 0)[:, None], AR_OFF_TRACK[None, :], cfg["x0"][None, :]).astype(np.float32)
    orc, twin = oracle_twin(cfg, n)
    want = np.empty(n, np.float32)
    want_crash = np.empty(n, np.int32)
    for x0, rows in ((AR_OFF_TRACK, np.arange(0, n, 2)), (cfg["x0"], np.arange(1, n, 2))):
        c, v = oracle_costs(orc, twin, x0, u)
        want[rows] = c[rows]
        want_crash[rows] = oracle_last_crash(orc, twin, x0, v[rows])
    with env_override(MPPI_AMD_FINALIZE_FORM=form):
        eng = make_engine(cfg)
        cost, crash = eng.evaluate_controls(starts, u)
        # and from the off-track start alone: crashed by the third step, not yet after the first
        all_off, crash_off = eng.evaluate_controls(AR_OFF_TRACK, u)
        eng.close()
    assert np.array_equal(crash, want_crash)
    assert (crash[0::2] == 1).all() and (crash[1::2] == 0).all()
    assert int(ulp_diff(cost, want).max()) == 0
    assert (crash_off == 1).all() and int(ulp_diff(all_off[0::2], want[0::2]).max()) == 0


# ------------------------------------------------------------------ 4. a control deadband is applied once ---------------
@pytest.mark.parametrize("name", ["cartpole", "racer_dubins"])
def test_control_deadband_is_applied_once(gpu, name):
    make_cfg, _, _, _, _ = FORMS[name]
    T, n = 9, 67
    cfg = make_cfg(T)
    C_ = len(cfg["std_dev"])
    band = np.array([0.7, 0.2][:C_], np.float32)
    amplitude = 7.0 if name == "cartpole" else 1.5
    u = np.random.default_rng(8).uniform(-amplitude, amplitude, (n, T, C_)).astype(np.float32)
    orc, twin = oracle_twin(cfg, n)
    orc.set_control_deadband(band)
    want, v = oracle_costs(orc, twin, cfg["x0"], u)
    twice, _ = oracle_costs(orc, twin, cfg["x0"], v)  # what a second application would give
    assert (ulp_diff(want, twice) > 0).sum() > n // 2
    eng = make_engine(cfg)
    eng.setControlDeadbands(band)
    cost, _ = eng.evaluate_controls(cfg["x0"], u)
    eng.close()
    assert int(ulp_diff(cost, want).max()) == 0


# ------------------------------------------------------------------ 5. consistent with the rollout and replay kernels -----
@pytest.mark.parametrize("name,K,T", [("cartpole", 200, 5), ("double_integrator", 130, 17), ("autorally_nn-wave", 65, 9),
                                      ("autorally_nn-rep", 130, 17)])
def test_saved_samples_give_the_rollout_kernels_costs_and_the_replayed_fold(gpu, name, K, T):
    make_cfg, _, form, _, _ = FORMS[name]
    cfg = make_cfg(T)
    cfg["K"] = K
    assert not np.any(cfg["control_cost_coeff"])  # a zero likelihood-ratio coefficient
    eng = make_engine(cfg, save_samples=True)
    eng.injectNoise(host_noise(1, K, T, eng.CONTROL_DIM)[0])
    costs = eng.rolloutCosts(cfg["x0"], 1)[0]
    v = eng.getSampledControls()[0]
    rows = np.unique(np.concatenate([np.arange(0, K, 7), [K - 2, K - 1]])).astype(np.int32)
    with env_override(MPPI_AMD_FINALIZE_FORM=form):
        cost, crash = eng.evaluate_controls(cfg["x0"], v[rows])
        _, step, step_crash = eng.replay_rollouts(rows)
    assert int(ulp_diff(cost, costs[rows]).max()) == 0
    assert int(ulp_diff(cost, fold_step_costs(step)).max()) == 0
    assert np.array_equal(crash, step_crash[:, -1])
    # nothing the controller computes depends on the call: the costs are still the rollouts'
    assert np.array_equal(eng.getSampledCostSeq()[0].view(np.int32), costs.view(np.int32))
    eng.close()


# ------------------------------------------------------------------ 6. a NaN stays in its row ----------------------------
def test_a_nan_gives_a_nan_cost_in_its_row_only(gpu):
    """the NaN is in one row's initial state: nothing constrains a state, it reaches every step cost of that row and of no other"""
    T, n, bad = 5, 67, 17
    cfg = di_cfg(K=64, T=T, tube=False)
    u = draw_rows("double_integrator", cfg, n, T, 2.0)
    starts = np.repeat(cfg["x0"][None, :], n, axis=0)
    starts[bad, 2] = np.nan
    orc, twin = oracle_twin(cfg, n)
    want, _ = oracle_costs(orc, twin, cfg["x0"], u)
    assert np.isnan(oracle_costs(orc, twin, starts[bad], u)[0]).all()
    eng = make_engine(cfg)
    cost, _ = eng.evaluate_controls(starts, u)
    eng.close()
    assert np.flatnonzero(np.isnan(cost)).tolist() == [bad]
    ok = np.arange(n) != bad
    assert int(ulp_diff(cost[ok], want[ok]).max()) == 0


def test_a_nan_control_is_constrained_as_the_rollout_kernel_constrains_it(gpu):
    """the base enforceConstraints rule is fminf(fmaxf(lower, u), upper): a NaN control becomes the lower bound, here and in the
    rollout kernel and the oracle alike — the row's cost is a number, the oracle's, and no other row changes"""
    T, n, bad = 5, 67, 17
    cfg = cartpole_cfg(K=64, T=T, soft=True)
    u = draw_rows("cartpole", cfg, n, T, 4.0)
    clean = u.copy()
    u[bad, 1, 0] = np.nan
    clean[bad, 1, 0] = -5.0
    orc, twin = oracle_twin(cfg, n)
    want, v = oracle_costs(orc, twin, cfg["x0"], u)
    assert v[bad, 1, 0] == -5.0 and np.isfinite(want).all()
    eng = make_engine(cfg)
    cost, _ = eng.evaluate_controls(cfg["x0"], u)
    same, _ = eng.evaluate_controls(cfg["x0"], clean)
    eng.close()
    assert int(ulp_diff(cost, want).max()) == 0
    assert np.array_equal(cost.view(np.int32), same.view(np.int32))


# ------------------------------------------------------------------ 7. every controller kind, sharded, fresh ------------
def test_robust_handle_evaluates_the_plain_model(gpu):
    cfg = rm_cfg("di", K=512, T=5)
    eng, _, _ = make_pair(cfg)  # no iteration, no gains: no feedback term is involved
    u = draw_rows("double_integrator", cfg, 67, 5, 4.0)
    check_against_the_oracle(eng, cfg, cfg["x0"], u, tag="robust")
    eng.close()


def test_tube_and_colored_handles_evaluate(gpu):
    from common import colored_cartpole
    cfg = di_cfg(K=64, T=5, tube=True)
    eng = make_engine(cfg)
    check_against_the_oracle(eng, cfg, cfg["x0"], draw_rows("double_integrator", cfg, 67, 5, 2.0), tag="tube")
    eng.close()
    cfg = colored_cartpole(K=64, T=9)
    eng = make_engine(cfg)
    assert eng.sampler == m.MPPI_SAMPLER_COLORED
    plain = dict(cfg)
    del plain["colored"]
    check_against_the_oracle(eng, plain, cfg["x0"], draw_rows("cartpole", cfg, 67, 9, 4.0), tag="colored")
    eng.close()


def test_rank_one_of_a_sharded_handle_evaluates_locally(gpu):
    cfg = cartpole_cfg(K=200, T=5, soft=True)
    eng = make_engine(cfg, rank=1, world_size=2)
    assert eng.num_rollouts_local == 100 and eng.rollout_offset == 100
    u = draw_rows("cartpole", cfg, 131, 5, 4.0)  # more rows than the rank has rollouts: the call does not depend on K
    cost, crash, _ = check_against_the_oracle(eng, cfg, cfg["x0"], u, tag="sharded")
    whole = make_engine(cfg)
    cost1, crash1 = whole.evaluate_controls(cfg["x0"], u)
    assert np.array_equal(cost.view(np.int32), cost1.view(np.int32)) and np.array_equal(crash, crash1)
    eng.close()
    whole.close()


def test_device_side_refusals_and_the_python_shape_checks(gpu):
    cfg = cartpole_cfg(K=64, T=3, soft=True)
    eng = make_engine(cfg)
    u = draw_rows("cartpole", cfg, 4, 3, 4.0)
    with pytest.raises(m.MPPIError) as e:
        eng.evaluate_controls(np.zeros((2, 4), np.float32), u)
    assert e.value.status == m.MPPI_ERR_INVALID_ARG and "x0_count = 2 is neither 1" in str(e.value)
    with pytest.raises(m.MPPIError) as e:
        eng.evaluate_controls(cfg["x0"], np.zeros((0, 3, 1), np.float32))
    assert e.value.status == m.MPPI_ERR_INVALID_ARG and "n = 0 is outside [1, 65536]" in str(e.value)
    with pytest.raises(m.MPPIError) as e:
        eng.evaluate_controls(cfg["x0"], np.zeros(5, np.float32))
    assert e.value.status == m.MPPI_ERR_INVALID_ARG
    with pytest.raises(m.MPPIError) as e:
        eng.warm_start(cfg["x0"], u, hysteresis=-1.0)
    assert e.value.status == m.MPPI_ERR_INVALID_ARG and "finite and >= 0" in str(e.value)
    # a model whose bulk data are missing says so instead of running
    bare = m.VanillaMPPIController("autorally_nn", 64, 3, 0.02, 1.0, 0.0, 1, seed=SEED)
    with pytest.raises(m.MPPIError) as e:
        bare.evaluate_controls(np.zeros(7, np.float32), np.zeros((1, 3, 2), np.float32))
    assert e.value.status == m.MPPI_ERR_STATE
    bare.close()
    eng.close()


# ------------------------------------------------------------------ 8. warm start ---------------------------------------
def _warm_case(cfg, seed=4):
    """four drawn sequences ordered by their evaluated cost, worst first: (rows, costs)"""
    eng = make_engine(cfg)
    T, C_ = cfg["T"], len(cfg["std_dev"])
    u = np.random.default_rng(seed).uniform(-2.0, 2.0, (4, T, C_)).astype(np.float32)
    cost, _ = eng.evaluate_controls(cfg["x0"], u)
    eng.close()
    order = np.argsort(-cost, kind="stable")
    assert np.unique(cost).size == 4
    return u[order], cost[order]


def _fresh(cfg, current, eps):
    eng = make_engine(cfg)
    eng.updateImportanceSampler(current)
    eng.injectNoise(eps)
    return eng


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.int32), np.ascontiguousarray(b, np.float32).view(np.int32))


def test_warm_start_installs_the_cheapest_candidate_beyond_the_hysteresis(gpu):
    cfg = cartpole_cfg(K=200, T=9, soft=True)
    rows, costs = _warm_case(cfg)
    current, candidates = rows[0], rows[[2, 3, 1]]  # the cheapest candidate is index 1
    eps = host_noise(1, 200, 9, 1)[0]
    gap = np.float32(costs[0] - costs[3])
    hysteresis = float(gap / np.float32(2))
    eng, twin = _fresh(cfg, current, eps), _fresh(cfg, current, eps)
    chosen, got = eng.warm_start(cfg["x0"], candidates, hysteresis)
    assert _same_bits(got, costs[[0, 2, 3, 1]])
    assert chosen == 1 == choice_reference(got, hysteresis)
    assert _same_bits(eng.getControlSeq(), candidates[1])
    twin.updateImportanceSampler(candidates[1])
    eng.computeControl(cfg["x0"], 1)
    twin.computeControl(cfg["x0"], 1)
    assert _same_bits(eng.getControlSeq(), twin.getControlSeq())
    assert _same_bits(eng.getSampledCostSeq(), twin.getSampledCostSeq())
    # after a slide the current sequence is the slid one
    eng.slideControlSequence(1)
    _, after = eng.warm_start(cfg["x0"], candidates, 1e30)
    assert _same_bits(after[:1], eng.evaluate_controls(cfg["x0"], eng.getControlSeq()[None])[0])
    eng.close()
    twin.close()


def test_warm_start_keeps_the_current_sequence_within_the_hysteresis(gpu):
    cfg = cartpole_cfg(K=200, T=9, soft=True)
    rows, costs = _warm_case(cfg)
    current, candidates = rows[0], rows[[2, 3, 1]]
    eps = host_noise(1, 200, 9, 1)[0]
    gap = np.float32(costs[0] - costs[3])
    assert np.float32(costs[0] - gap) == costs[3]  # (costs within a factor of two of each other: both differences are exact)
    eng, twin = _fresh(cfg, current, eps), _fresh(cfg, current, eps)
    for hysteresis in (float(gap), float(gap * np.float32(2))):  # exactly the gap: the compare is strict
        chosen, got = eng.warm_start(cfg["x0"], candidates, hysteresis)
        assert chosen == -1 == choice_reference(got, hysteresis)
        assert _same_bits(got, costs[[0, 2, 3, 1]])
        assert _same_bits(eng.getControlSeq(), current)
    eng.computeControl(cfg["x0"], 1)
    twin.computeControl(cfg["x0"], 1)
    assert _same_bits(eng.getControlSeq(), twin.getControlSeq())
    assert _same_bits(eng.getSampledCostSeq(), twin.getSampledCostSeq())
    # a current sequence that costs NaN gives way to any number, whatever the hysteresis
    # (finite controls of 1e30 on the double integrator, which has no control ranges: from the second step on the angular
    # momentum is inf - inf.  A NaN control would not do: the constraint rule turns it into the lower bound.)
    free_cfg = di_cfg(K=64, T=9, tube=False)
    free = make_engine(free_cfg)
    di_rows = np.random.default_rng(6).uniform(-1, 1, (2, 9, 2)).astype(np.float32)
    bad = np.full((9, 2), 1e30, np.float32)
    orc, twin_cfg = oracle_twin(free_cfg, 3)
    want, _ = oracle_costs(orc, twin_cfg, free_cfg["x0"], np.concatenate([bad[None], di_rows]))
    assert np.isnan(want[0]) and np.isfinite(want[1:]).all()
    free.updateImportanceSampler(bad)
    chosen, got = free.warm_start(free_cfg["x0"], di_rows, 1e30)
    assert np.isnan(got[0]) and int(ulp_diff(got[1:], want[1:]).max()) == 0 and chosen == choice_reference(got, 1e30) >= 0
    assert _same_bits(free.getControlSeq(), di_rows[chosen])
    free.close()
    eng.close()
    twin.close()


def test_warm_start_on_a_tube_handle_installs_both_trajectories(gpu):
    cfg = di_cfg(K=200, T=9, tube=True)
    rows, costs = _warm_case(cfg)
    eng = _fresh(cfg, rows[0], host_noise(1, 200, 9, 2)[0])
    chosen, got = eng.warm_start(cfg["x0"], rows[[1, 3, 2]], 0.0)
    assert chosen == 1 and _same_bits(got, costs[[0, 1, 3, 2]])
    assert _same_bits(eng.getControlSeq(), rows[3]) and _same_bits(eng.getNominalControlSeq(), rows[3])
    eng.close()


def test_warm_start_is_refused_on_a_robust_handle(gpu):
    cfg = rm_cfg("di", K=512, T=5)
    eng, _, _ = make_pair(cfg)
    before = eng.getControlSeq()
    with pytest.raises(m.MPPIError) as e:
        eng.warm_start(cfg["x0"], np.zeros((2, 5, 2), np.float32))
    assert e.value.status == m.MPPI_ERR_UNSUPPORTED and ROBUST_TEXT in str(e.value)
    assert _same_bits(eng.getControlSeq(), before)
    eng.close()


# ------------------------------------------------------------------ 9. the device block goes with the handle --------------
def test_live_allocations_return_to_their_starting_count(gpu, lib):
    def live():
        n, b = C.c_int64(), C.c_int64()
        assert lib.mppi_debug_live_allocations(C.byref(n), C.byref(b)) == m.MPPI_OK
        return n.value, b.value

    gc.collect()  # an earlier test's handle nobody closed goes now, not between the two counts
    start = live()
    cfg = cartpole_cfg(K=64, T=9, soft=True)
    eng = make_engine(cfg)
    created = live()
    eng.evaluate_controls(cfg["x0"], draw_rows("cartpole", cfg, 3, 9, 4.0))
    small = live()
    assert small[0] == created[0] + 1 and small[1] > created[1]
    eng.evaluate_controls(cfg["x0"], draw_rows("cartpole", cfg, 3, 9, 4.0))
    assert live() == small  # the block is kept
    eng.warm_start(cfg["x0"], draw_rows("cartpole", cfg, 300, 9, 4.0))
    grown = live()
    assert grown[0] == small[0] and grown[1] > small[1]  # grown in place: one block
    eng.close()
    assert live() == start
