"""mppi_top_rollouts and mppi_replay_rollouts on the device: the selection against the pure-Python reference, the replayed
outputs, step costs and crash flags against the oracle at 0 ulp, the optimal sequence against the finalize pass, the other
samplers, a K-sharded handle, the refusals.  Small shapes: (K, T) = (65, 3), (200, 5), (1049, 9), (130, 17) cover partial waves
and blocks.  y_out[t] is the output AFTER step t: row t + 1 of the oracle's / the finalize pass's output trajectory, whose row 0
is the output before the first step; the last replayed row is one oracle step past that trajectory's end.

Measured on an MI355X: every comparison below at 0 ulp."""
import numpy as np
import pytest

import mppi_generic_amd as m
from common import (SEED, autorally_cfg, cartpole_cfg, cartpole_cfg_lr, colored_cartpole, di_cfg, host_noise, make_engine,
                    make_oracle, make_pair, racer_cfg, rm_cfg, ulp_diff)
from kernel_forms import env_override
from replay_cases import boundary_rows, fold_step_costs, oracle_row, selection_reference

pytestmark = pytest.mark.gpu

KT = [(65, 3), (200, 5), (1049, 9), (130, 17)]
NS = (1, 7, 64, 256)
AR_OFF_TRACK = np.array([-12.0, 4.85, 1.57, 0.0, 8.0, 0.0, 0.0], np.float32)  # leaves the track after its first step


def _run(cfg, x0=None, compute=True, **kw):
    """an engine with saved samples and injected noise after one computeControl (or one rolloutCosts), and its oracle"""
    eng = make_engine(cfg, save_samples=True, **kw)
    C = eng.CONTROL_DIM
    eng.injectNoise(host_noise(1, cfg["K"], cfg["T"], C)[0][eng.rollout_offset:eng.rollout_offset + eng.num_rollouts_local])
    x0 = cfg["x0"] if x0 is None else x0
    if compute:
        eng.computeControl(x0, 1)
    else:
        eng.rolloutCosts(x0, 1)
    return eng, make_oracle(cfg)


def _check_selection(eng, system=0):
    costs = eng.getSampledCostSeq()[system]
    for n in [n for n in NS if n <= costs.size]:
        idx, val = eng.top_rollouts(n, system)
        ref_idx, ref_val = selection_reference(costs, n)
        assert np.array_equal(idx, ref_idx), (n, idx[:8], ref_idx[:8])
        assert np.array_equal(val.view(np.int32), ref_val.view(np.int32)), n
    return costs


# ------------------------------------------------------------------ 1. selection -----------------------------------------
@pytest.mark.parametrize("K,T", KT[:3])
@pytest.mark.parametrize("model", ["cartpole", "double_integrator"])
def test_selection_after_real_iterations(gpu, model, K, T):
    cfg = cartpole_cfg(K=K, T=T, soft=True) if model == "cartpole" else di_cfg(K=K, T=T, tube=False)
    eng, _ = _run(cfg)
    costs = _check_selection(eng)
    assert np.isfinite(costs).all()


def test_selection_large_k(gpu):
    eng, _ = _run(di_cfg(K=16384, T=3, tube=False))
    _check_selection(eng)


def test_selection_on_a_tube_handle_takes_each_system(gpu):
    cfg = di_cfg(K=200, T=5, tube=True)
    eng, _ = _run(cfg, x0=np.stack([cfg["x0"], cfg["x0"] + np.float32(0.3)]), compute=False)
    c0, c1 = _check_selection(eng, 0), _check_selection(eng, 1)
    assert not np.array_equal(c0, c1)


@pytest.mark.parametrize("K,T", [(200, 5), (1049, 9)])
def test_selection_with_exact_ties(gpu, K, T):
    """no velocity cost: a rollout's cost is its number of crashed steps times crash_cost / T"""
    cfg = di_cfg(K=K, T=T, tube=False)
    cfg["cost"].velocity_cost = 0
    cfg["x0"] = np.array([2.12, 0.0, 0.0, 1.0], np.float32)  # close to the outer edge of the track
    cfg["std_dev"] = [3.0, 3.0]
    eng, _ = _run(cfg, compute=False)
    costs = _check_selection(eng)
    assert np.unique(costs).size <= T + 1 < K


def test_selection_with_infinite_and_nan_costs(gpu):
    cfg = di_cfg(K=1049, T=9, tube=False)
    cfg["cost"].crash_cost = float("inf")
    cfg["x0"] = np.array([2.12, 0.0, 0.0, 1.0], np.float32)
    cfg["std_dev"] = [3.0, 3.0]
    eng = make_engine(cfg, save_samples=True)
    eps = host_noise(1, 1049, 9, 2)[0]
    eps[77] = np.inf  # an infinite control: inf - inf in the angular momentum, a NaN cost
    eng.injectNoise(eps)
    eng.rolloutCosts(cfg["x0"], 1)
    costs = _check_selection(eng)
    assert np.isnan(costs[77]) and np.isposinf(costs).sum() > 1 and np.isfinite(costs).sum() > 1
    # the NaN is last, behind every +inf
    order, _ = selection_reference(costs, costs.size)
    assert order[-np.isnan(costs).sum():].tolist() == np.flatnonzero(np.isnan(costs)).tolist()


# ------------------------------------------------------------------ 2. replay against the oracle -------------------------
def _replay_case(name):
    if name == "cartpole":
        return cartpole_cfg(K=65, T=3, soft=True), {}, None
    if name == "double_integrator":
        return di_cfg(K=200, T=5, tube=False), {}, None
    if name == "double_integrator-tube":
        return di_cfg(K=130, T=17, tube=True), {}, None
    if name == "racer_dubins":
        return racer_cfg(K=1049, T=9), {}, None
    if name == "autorally_nn-wave":
        return autorally_cfg(K=200, T=5), {}, None
    if name == "autorally_nn-rep":
        return autorally_cfg(K=130, T=17), {}, "rep"
    raise KeyError(name)


@pytest.mark.parametrize("name", ["cartpole", "double_integrator", "double_integrator-tube", "racer_dubins", "autorally_nn-wave",
                                  "autorally_nn-rep"])
def test_replay_equals_the_oracle(gpu, name):
    cfg, kw, form = _replay_case(name)
    tube = cfg["D"] == 2
    x0 = np.stack([cfg["x0"], cfg["x0"] + np.float32(0.25)]) if tube else cfg["x0"]
    eng, orc = _run(cfg, x0=x0, compute=not tube, **kw)  # (a Tube call may move the nominal system's start afterwards)
    v = eng.getSampledControls()
    rows = boundary_rows(cfg["K"])
    with env_override(MPPI_AMD_FINALIZE_FORM=form):
        for system in range(cfg["D"]):
            y, cost, crash = eng.replay_rollouts(rows, system)
            x0s = x0[system] if tube else x0
            ref = [oracle_row(orc, cfg, x0s, v[system, k]) for k in rows]
            assert int(ulp_diff(y, np.stack([r[0] for r in ref])).max()) == 0, (name, system)
            assert int(ulp_diff(cost, np.stack([r[1] for r in ref])).max()) == 0, (name, system)
            assert np.array_equal(crash, np.stack([r[2] for r in ref]))
            assert (np.diff(crash, axis=1) >= 0).all()
            # and the fold of the step costs is the rollout's trajectory cost
            assert int(ulp_diff(fold_step_costs(cost), eng.getSampledCostSeq()[system, rows]).max()) == 0, (name, system)


@pytest.mark.parametrize("form", [None, "rep"])
def test_replay_keeps_the_sticky_crash_status(gpu, form):
    cfg = autorally_cfg(K=65, T=9)
    eng, orc = _run(cfg, x0=AR_OFF_TRACK)
    v = eng.getSampledControls()
    rows = boundary_rows(65)
    with env_override(MPPI_AMD_FINALIZE_FORM=form):
        y, cost, crash = eng.replay_rollouts(rows)
    ref = [oracle_row(orc, cfg, AR_OFF_TRACK, v[0, k]) for k in rows]
    assert np.array_equal(crash, np.stack([r[2] for r in ref]))
    assert crash.min() == 0 and crash.max() == 1 and (np.diff(crash, axis=1) >= 0).all()
    assert int(ulp_diff(y, np.stack([r[0] for r in ref])).max()) == 0
    assert int(ulp_diff(cost, np.stack([r[1] for r in ref])).max()) == 0


@pytest.mark.parametrize("model", ["cartpole", "double_integrator"])
def test_step_costs_fold_to_the_trajectory_costs_with_a_control_cost(gpu, model):
    """non-zero control_cost_coeff, alpha and nominal control: the likelihood-ratio term is in every step cost"""
    if model == "cartpole":
        cfg = cartpole_cfg_lr(K=1049, T=9)
    else:
        cfg = di_cfg(K=130, T=17, tube=False)
        cfg["control_cost_coeff"], cfg["alpha"], cfg["ranges"] = [0.3, 0.2], 0.1, [[-3.0, 3.0], [-3.0, 3.0]]
    K, T = cfg["K"], cfg["T"]
    eng = make_engine(cfg, save_samples=True)
    C = eng.CONTROL_DIM
    mean = (0.4 * np.sin(np.arange(T * C, dtype=np.float32))).reshape(T, C).astype(np.float32)
    eng.updateImportanceSampler(mean)
    eng.injectNoise(host_noise(1, K, T, C)[0])
    costs = eng.rolloutCosts(cfg["x0"], 1)[0]
    rows = np.arange(min(K, 1024), dtype=np.int32) if K <= 1024 else np.concatenate([np.arange(1015), boundary_rows(K)]).astype(np.int32)
    _, step, _ = eng.replay_rollouts(rows)
    assert np.abs(step[:, :T]).max() > 0
    assert int(ulp_diff(fold_step_costs(step), costs[rows]).max()) == 0
    # the step costs themselves, against the oracle's state cost and the restated likelihood-ratio term
    orc = make_oracle(cfg)
    v = eng.getSampledControls()[0]
    term = None
    if model == "cartpole":
        coeff = np.float32(cfg["cost"].terminal_cost_coeff)
        term = lambda y: np.float32(np.float32(orc.state_cost(y, 0, 0)[0]) * coeff)  # noqa: E731
    some = boundary_rows(K)
    ref = np.stack([oracle_row(orc, cfg, cfg["x0"], v[k], mean, int(k), term)[1] for k in some])
    _, step_some, _ = eng.replay_rollouts(some)
    assert int(ulp_diff(step_some, ref).max()) == 0


# ------------------------------------------------------------------ 3. the optimal sequence ------------------------------
@pytest.mark.parametrize("model", ["cartpole", "racer_dubins", "autorally_nn"])
def test_index_minus_one_reproduces_the_output_sequence(gpu, model):
    """on a handle WITHOUT saved samples"""
    cfg = {"cartpole": cartpole_cfg(K=200, T=5, soft=True), "racer_dubins": racer_cfg(K=65, T=9),
           "autorally_nn": autorally_cfg(K=130, T=17)}[model]
    eng = make_engine(cfg)
    eng.injectNoise(host_noise(1, cfg["K"], cfg["T"], eng.CONTROL_DIM)[0])
    eng.computeControl(cfg["x0"], 1)
    y, cost, crash = eng.replay_rollouts([-1])
    out = eng.getTargetOutputSeq()
    assert int(ulp_diff(y[0, :-1], out[1:]).max()) == 0
    assert np.isfinite(cost).all() and cost.shape == (1, cfg["T"] + 1)
    with pytest.raises(m.MPPIError) as e:
        eng.replay_rollouts([-1, 0])
    assert e.value.status == m.MPPI_ERR_STATE and "save_samples" in str(e.value)


def test_index_minus_one_on_tube_is_the_nominal_trajectory(gpu):
    cfg = di_cfg(K=200, T=5, tube=True)
    eng = make_engine(cfg)
    eng.injectNoise(host_noise(1, 200, 5, 2)[0])
    eng.computeControl(cfg["x0"], 1)
    orc = make_oracle(cfg)
    for system, u in ((0, eng.getControlSeq()), (1, eng.getNominalControlSeq())):
        y, _, _ = eng.replay_rollouts([-1], system)
        # (the first call starts the nominal system at the measured state)
        assert int(ulp_diff(y[0], oracle_row(orc, cfg, cfg["x0"], u)[0]).max()) == 0, system
    assert int(ulp_diff(eng.replay_rollouts([-1], 0)[0][0, :-1], eng.getTargetOutputSeq()[1:]).max()) == 0


# ------------------------------------------------------------------ 4. the other samplers --------------------------------
def test_replay_on_an_nln_handle(gpu):
    cfg = cartpole_cfg(K=200, T=5, soft=True)
    eng = make_engine(cfg, save_samples=True, sampler=m.MPPI_SAMPLER_NLN)
    eng.computeControl(cfg["x0"], 1)
    orc = make_oracle(cfg)
    v, rows = eng.getSampledControls()[0], boundary_rows(200)
    y, cost, _ = eng.replay_rollouts(rows)
    ref = [oracle_row(orc, cfg, cfg["x0"], v[k]) for k in rows]
    assert int(ulp_diff(y, np.stack([r[0] for r in ref])).max()) == 0
    assert int(ulp_diff(cost, np.stack([r[1] for r in ref])).max()) == 0


def test_replay_on_a_colored_handle(gpu):
    cfg = colored_cartpole(K=130, T=17)
    eng = make_engine(cfg, save_samples=True)
    assert eng.sampler == m.MPPI_SAMPLER_COLORED
    eng.computeControl(cfg["x0"], 1)
    orc = make_oracle(cfg)
    v, rows = eng.getSampledControls()[0], boundary_rows(130)
    y, cost, _ = eng.replay_rollouts(rows)
    ref = [oracle_row(orc, cfg, cfg["x0"], v[k]) for k in rows]
    assert int(ulp_diff(y, np.stack([r[0] for r in ref])).max()) == 0
    assert int(ulp_diff(cost, np.stack([r[1] for r in ref])).max()) == 0
    assert int(ulp_diff(fold_step_costs(cost), eng.getSampledCostSeq()[0, rows]).max()) == 0


# ------------------------------------------------------------------ 5. a K-sharded handle --------------------------------
def test_local_indices_address_local_rows_on_a_sharded_handle(gpu):
    cfg = cartpole_cfg(K=200, T=5, soft=True)
    eng, orc = _run(cfg, compute=False, rank=1, world_size=2)
    KL = eng.num_rollouts_local
    assert KL < 200 and eng.rollout_offset > 0
    v = eng.getSampledControls()[0]
    assert v.shape[0] == KL
    rows = np.array([0, 1, KL // 2, KL - 2, KL - 1], np.int32)
    y, cost, _ = eng.replay_rollouts(rows)
    ref = [oracle_row(orc, cfg, cfg["x0"], v[k]) for k in rows]
    assert int(ulp_diff(y, np.stack([r[0] for r in ref])).max()) == 0
    assert int(ulp_diff(fold_step_costs(cost), eng.getSampledCostSeq()[0, rows]).max()) == 0
    _check_selection(eng)
    for call in (lambda: eng.replay_rollouts([KL]), lambda: eng.top_rollouts(KL + 1)):
        with pytest.raises(m.MPPIError) as e:
            call()
        assert e.value.status == m.MPPI_ERR_INVALID_ARG


# ------------------------------------------------------------------ 6. refusals ------------------------------------------
def _refused(call, status, text):
    with pytest.raises(m.MPPIError) as e:
        call()
    assert e.value.status == status and text in str(e.value), str(e.value)


def test_refusals(gpu):
    cfg = cartpole_cfg(K=65, T=3, soft=True)
    fresh = make_engine(cfg, save_samples=True)
    _refused(lambda: fresh.top_rollouts(1), m.MPPI_ERR_STATE, "no iteration has run on this handle yet")
    _refused(lambda: fresh.replay_rollouts([0]), m.MPPI_ERR_STATE, "no iteration has run on this handle yet")
    plain = make_engine(cfg)
    plain.rolloutCosts(cfg["x0"], 1)
    _refused(lambda: plain.replay_rollouts([0]), m.MPPI_ERR_STATE, "handle was created without save_samples")
    _refused(lambda: plain.replay_rollouts([-1]), m.MPPI_ERR_STATE, "index -1 is the control sequence of a mppi_compute_control")
    assert plain.top_rollouts(3)[0].size == 3
    eng, _ = _run(cfg)
    _refused(lambda: eng.top_rollouts(1, system=1), m.MPPI_ERR_INVALID_ARG, "system 0, or 1 (the nominal system)")
    _refused(lambda: eng.replay_rollouts([0], system=2), m.MPPI_ERR_INVALID_ARG, "system 0, or 1 (the nominal system)")
    _refused(lambda: eng.top_rollouts(0), m.MPPI_ERR_INVALID_ARG, "is outside [1, 65]")
    _refused(lambda: eng.top_rollouts(66), m.MPPI_ERR_INVALID_ARG, "is outside [1, 65]")
    _refused(lambda: eng.replay_rollouts([0, 65]), m.MPPI_ERR_INVALID_ARG, "rollout_idx[1] = 65 is outside [-1, 65)")
    _refused(lambda: eng.replay_rollouts([-2]), m.MPPI_ERR_INVALID_ARG, "rollout_idx[0] = -2")
    _refused(lambda: eng.replay_rollouts(np.zeros(0, np.int32)), m.MPPI_ERR_INVALID_ARG, "n = 0 is outside [1, 1024]")
    _refused(lambda: eng.replay_rollouts(np.zeros(1025, np.int32)), m.MPPI_ERR_INVALID_ARG, "n = 1025 is outside [1, 1024]")
    big = make_engine(cartpole_cfg(K=1049, T=3, soft=True))
    big.rolloutCosts(cfg["x0"], 1)
    _refused(lambda: big.top_rollouts(257), m.MPPI_ERR_INVALID_ARG, "is outside [1, 256]")
    rob, _, _ = make_pair(rm_cfg("di", K=512, T=5), save_samples=True)
    _refused(lambda: rob.replay_rollouts([0]), m.MPPI_ERR_UNSUPPORTED, "Robust MPPI handle carry the feedback term")


def test_sampled_trajectories_forms_the_reference_list(gpu):
    cfg = cartpole_cfg(K=1049, T=9, soft=True)
    eng, _ = _run(cfg)
    out = eng.sampled_trajectories(top_n=7, fraction=0.02, seed=5)
    n_rand = int(0.02 * 1049)
    assert out["indices"][0] == -1 and out["indices"].size == 1 + n_rand + 7
    top_idx, top_cost = eng.top_rollouts(7)
    assert np.array_equal(out["indices"][-7:], top_idx) and np.array_equal(out["top_costs"], top_cost)
    assert out["outputs"].shape == (out["indices"].size, 9, eng.OUTPUT_DIM)
    assert int(ulp_diff(fold_step_costs(out["costs"][-7:]), top_cost).max()) == 0
    assert int(ulp_diff(out["outputs"][0, :-1], eng.getTargetOutputSeq()[1:]).max()) == 0
