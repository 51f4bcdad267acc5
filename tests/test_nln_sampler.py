"""The NLN (normal-log-normal, log-MPPI) sampling distribution: include/mppi_amd/sampling_distributions/nln.hpp.

For row element e = t * C + c of global rollout k and noise stream s (0, or the distribution index with independent noise)
    eps' = z1 * det::exp(std_dev[c] * z2),   z1 = Philox stream s, z2 = Philox stream 16 + s, same (generation, k, quad, lane)
and everything downstream of eps' is the Gaussian sampler's code.  The oracle takes injected noise, and pyoracle exposes the
Philox normals per stream and det::exp, so the expected eps' is composed on the host (nln_noise below) and handed to the
un-modified oracle: parity is then a statement about the engine's draw — all three draw paths (in-loop drawQuad, the row
pre-fill, Robust MPPI's sampleAt) — and about nothing else.

Bars: sampled costs 0 ulp and u* within 1e-5 of the oracle (the project's standing bars); the moment test's bounds are 4
standard errors of the analytic moments of z * exp(sigma z'), E[e^2] = exp(2 sigma^2), Var[e^2] = 3 exp(8 sigma^2) -
exp(4 sigma^2), E[e] = 0, Var[e] = exp(2 sigma^2).

Two consecutive calls per parity case, so the generation counter advances.  The handles run the reference-order reduction
(as the exact handle of tests/test_kernel_sequence.py): with the fused merge u* differs from the oracle's by rounding, the
second call would sample around another mean and its costs could not be held to 0 ulp.
"""
import functools

import numpy as np
import pytest

import mppi_generic_amd as m
import pyoracle as po
from common import SEED, U_TOL, autorally_cfg, cartpole_cfg, cartpole_cfg_lr, di_cfg, host_noise, make_engine, robust_cfg, ulp_diff
from kernel_forms import KT, check_against_oracle, compute_once, make_handles

NLN = getattr(m, "MPPI_SAMPLER_NLN", 2)
NLN_STREAM_BASE = 16
MPPI_NOISE_ROCRAND_HOST = 2

assert {(1, 1), (63, 2), (65, 3), (1049, 9)} <= set(KT)


def nln_noise(seed, g, K, T, C, sigma, stream=0, k_begin=0, k_end=None):
    """eps'[K][T][C] of generation g composed on the host from the oracle's Philox normals and det::exp (func 2)"""
    sigma = np.asarray(sigma, np.float32).reshape(-1)[:C]
    z1 = po.philox_normal(seed, g, K, T, C, k_begin, k_end, stream=stream)
    z2 = po.philox_normal(seed, g, K, T, C, k_begin, k_end, stream=NLN_STREAM_BASE + stream)
    arg = (sigma[None, None, :] * z2).astype(np.float32)
    return (z1 * po.det_eval(2, arg).reshape(z1.shape)).astype(np.float32)


# ------------------------------------------------------------------ 1: CPU, no device ----------------------------------
def test_describe_model_lists_the_four_nln_registrations(lib):
    c = m.describe_model("cartpole", NLN)
    assert c is not None
    assert c["shapes"] == m.describe_model("cartpole")["shapes"]
    assert c["pipeline"] and c["streamed_merge"] and c["rows_in_hbm"] and c["pipeline_fold"] and not c["rmppi"]
    assert c["replicated_lane_shapes"] == []
    d = m.describe_model("double_integrator", NLN)
    assert d["shapes"] == m.describe_model("double_integrator")["shapes"]
    assert (64, 1, 1) in d["shapes"] and (64, 1, 2) in d["shapes"]
    assert d["pipeline"] and d["pipeline_fold"] and d["streamed_merge"] and not d["rmppi"]
    r = m.describe_model("double_integrator_robust", NLN)
    assert r["rmppi"] and r["rmppi_pipeline"] and r["pipeline"]
    a = m.describe_model("autorally_nn", NLN)
    assert a["replicated_lane_shapes"] == [(64, 4, 1), (32, 4, 1)] and (16, 8, 1) in a["shapes"]
    assert not a["pipeline"] and not a["rmppi"]
    assert m.describe_model("racer_dubins", NLN) is None
    # the NLN registrations add no model name
    assert len(m.list_models()) == len(set(m.list_models()))


def test_host_composed_noise_has_the_moments_of_the_definition():
    """the oracle-side composition the parity tests inject, at the moment test's shape: within 4 standard errors of the
    analytic moments, and plain Gaussian noise is far outside"""
    K, T, s = 4096, 8, 0.5
    n = (K - 1) * T
    m2, se2 = np.exp(2 * s * s), np.sqrt((3 * np.exp(8 * s * s) - np.exp(4 * s * s)) / n)
    for g in (0, 1):
        e = nln_noise(SEED, g, K, T, 1, [s])[1:].astype(np.float64)
        assert abs((e * e).mean() - m2) <= 4 * se2
        assert abs(e.mean()) <= 4 * np.sqrt(m2 / n)
    z = po.philox_normal(SEED, 0, K, T, 1)[1:].astype(np.float64)
    assert abs((z * z).mean() - m2) > 25 * se2


# ------------------------------------------------------------------ 2: GPU, parity on the in-kernel stream --------------
def _cartpole(K, T, D):
    cfg = cartpole_cfg_lr(K=K, T=T)
    cfg["std_dev"] = [0.8]  # the log-normal factor is exp(std_dev z'): 5.0 would saturate every control at its range
    cfg["D"] = D
    return cfg


def _di(K, T, D):
    cfg = di_cfg(K=K, T=T, tube=D == 2)
    cfg["std_dev"] = [0.7, 0.4]  # unequal: a swapped sigma index shows
    cfg["control_cost_coeff"] = [0.3, 0.2]
    return cfg


def _di_robust(K, T, D):
    cfg = robust_cfg(K=K, T=T, tube=True)
    cfg["std_dev"] = [0.7, 0.4]
    cfg["control_cost_coeff"] = [0.2, 0.1]
    return cfg


def _autorally(K, T, D):
    cfg = autorally_cfg(K=K, T=T)
    cfg["std_dev"] = [0.3, 0.2]
    cfg["D"] = D
    return cfg


def _case(id, build, ctl, kw, family, block, hbm=False, independent=False):
    return dict(id=id, build=build, controller=ctl, kw=kw, independent=independent,
                expect=dict(family=family, block=block, rows_in_hbm=hbm))


F, P, A = m.MPPI_KERNEL_FUSED, m.MPPI_KERNEL_PIPELINE, m.MPPI_KERNEL_AUTO
PARITY_CASES = [
    _case("cartpole-vanilla-fused64x1", _cartpole, "vanilla", dict(block_x=64, block_y=1, kernel_variant=F), "fused", (64, 1, 1)),
    _case("cartpole-vanilla-fused64x4-prefill", _cartpole, "vanilla", dict(block_x=64, block_y=4, kernel_variant=F), "fused", (64, 4, 1)),
    _case("cartpole-vanilla-pipeline", _cartpole, "vanilla", dict(block_x=64, block_y=1, kernel_variant=P), "pipeline", (64, 1, 1)),
    _case("double_integrator-vanilla-fused", _di, "vanilla", dict(block_x=64, block_y=1, kernel_variant=F), "fused", (64, 1, 1)),
    _case("double_integrator-vanilla-pipeline", _di, "vanilla", dict(block_x=64, block_y=1, kernel_variant=P), "pipeline", (64, 1, 1)),
    _case("double_integrator-tube-fused", _di, "tube", dict(block_x=64, block_y=1, kernel_variant=F), "fused", (64, 1, 2)),
    _case("double_integrator-tube-pipeline", _di, "tube", dict(block_x=64, block_y=1, kernel_variant=P), "pipeline", (64, 1, 2)),
    _case("double_integrator-tube-auto-fold", _di, "tube", dict(kernel_variant=A), "pipeline_fold", (32, 1, 2)),
    _case("double_integrator-tube-independent-noise", _di, "tube", dict(kernel_variant=A), "pipeline_fold", (32, 1, 2),
          independent=True),
    _case("double_integrator_robust-robust-fused", _di_robust, "robust", dict(block_x=64, kernel_variant=F), "rmppi", (64, 1, 2)),
    _case("double_integrator_robust-robust-pipeline", _di_robust, "robust", dict(kernel_variant=P), "rmppi_pipeline", (64, 1, 2),
          hbm=True),
    _case("autorally_nn-vanilla-pipeline-rep", _autorally, "vanilla", dict(block_x=64, block_y=4, kernel_variant=P), "pipeline_rep",
          (64, 4, 1)),
]


_make = functools.partial(make_handles, sampler=NLN)


def _noise_for(cfg, case, g, K, T, C):
    if case["independent"]:
        return np.stack([nln_noise(SEED, g, K, T, C, cfg["std_dev"], stream=d) for d in range(2)])
    return nln_noise(SEED, g, K, T, C, cfg["std_dev"])


def _assert_parity(eng, orc, ctl, tag):
    du = check_against_oracle(dict(controller=ctl), eng, orc, tag, show=True)
    assert du <= U_TOL, "%s: u* (or the nominal u*) differs from the oracle by %g" % (tag, du)


def _run_parity(case, K, T):
    ctl = case["controller"]
    tag0 = "%s K=%d T=%d" % (case["id"], K, T)
    if ctl == "robust" and K < 3:
        with pytest.raises(m.MPPIError) as e:  # RobustMPPIController needs at least 3 candidates x 1 sample
            _make(case, K, T)
        assert e.value.status == m.MPPI_ERR_INVALID_ARG, tag0
        return
    cfg, eng, orc, rob = _make(case, K, T)
    try:
        assert eng.sampler == NLN
        C = eng.CONTROL_DIM
        eng.setReductionMode(m.MPPI_REDUCTION_REFERENCE_ORDER)
        if case["independent"]:
            eng.setIndependentNoise(True)
            orc.set_independent_noise(True)
        eng.setSeed(SEED)
        gen = 0  # the engine's generation counter: one per rollout launch, one per Robust candidate evaluation
        for call in range(2):
            tag = "%s call %d" % (tag0, call)
            candidate_noise = None
            if ctl == "robust":
                if call > 0:  # (the first cycle has no nominal state yet and evaluates no candidates)
                    candidate_noise = _noise_for(cfg, case, gen, K, T, C)
                    gen += 1
            elif call > 0:
                eng.slideControlSequence(1)
                (orc.tube_slide if ctl == "tube" else orc.vanilla_slide)(1)
            eps = _noise_for(cfg, case, gen, K, T, C)[None]
            gen += 1
            # (the generator was seeded once, before the first call: no seed here)
            compute_once(case, [eng], orc, rob, cfg, 1, eps, True, None, candidate_noise=candidate_noise, first_cycle=call == 0)
            info = eng.getLaunchInfo()
            got = {k: info[k] for k in ("family", "block", "rows_in_hbm")}
            assert got == case["expect"], "%s: launched %s, the case expects %s" % (tag, got, case["expect"])
            _assert_parity(eng, orc, ctl, tag)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", PARITY_CASES, ids=[c["id"] for c in PARITY_CASES])
def test_nln_parity_with_the_oracle_on_the_in_kernel_stream(gpu, case):
    for K, T in KT:
        _run_parity(case, K, T)


# ------------------------------------------------------------------ 3: GPU, options ------------------------------------
PIPE = PARITY_CASES[2]
OPT_K, OPT_T = 300, 9


@pytest.mark.gpu
def test_nln_std_dev_decay_leaves_the_log_normal_sigma_undecayed(gpu):
    """std_dev_decay = 0.9 over 2 iterations: the second iteration's normal factor is scaled by 0.9 sigma, its log-normal
    factor still by exp(sigma z') — the host composition uses the undecayed sigma for both generations"""
    case = dict(PIPE, build=lambda K, T, D: dict(_cartpole(K, T, D), decay=0.9))
    cfg, eng, orc, _ = _make(case, OPT_K, OPT_T, num_iters=2)
    try:
        eng.setReductionMode(m.MPPI_REDUCTION_REFERENCE_ORDER)
        eng.setSeed(SEED)
        eps = np.stack([nln_noise(SEED, g, OPT_K, OPT_T, 1, cfg["std_dev"]) for g in range(2)])
        eng.computeControl(cfg["x0"], 1)
        orc.vanilla_compute_control(cfg["x0"], 1, eps)
        assert eng.getLaunchInfo()["family"] == "pipeline"
        _assert_parity(eng, orc, "vanilla", "decay 0.9, 2 iterations")
    finally:
        eng.close()


@pytest.mark.gpu
def test_nln_time_specific_std_dev_scales_the_normal_factor_only(gpu):
    cfg, eng, orc, _ = _make(PIPE, OPT_K, OPT_T)
    try:
        table = np.linspace(0.3, 1.5, OPT_T, dtype=np.float32).reshape(1, OPT_T, 1)
        eng.setTimeSpecificStdDev(table[0])
        orc.set_time_specific_std_dev(table)
        eng.setSeed(SEED)
        eps = nln_noise(SEED, 0, OPT_K, OPT_T, 1, cfg["std_dev"])[None]  # sigma of the log-normal: std_dev[c], not the table
        eng.computeControl(cfg["x0"], 1)
        orc.vanilla_compute_control(cfg["x0"], 1, eps)
        assert eng.getLaunchInfo()["family"] == "pipeline"
        _assert_parity(eng, orc, "vanilla", "time-specific sigma")
    finally:
        eng.close()


@pytest.mark.gpu
def test_nln_with_the_sample_rows_in_hbm(gpu, monkeypatch):
    monkeypatch.setenv("MPPI_AMD_ROWS_IN_HBM", "1")
    for case in (PARITY_CASES[0], PIPE):
        cfg, eng, orc, _ = _make(case, OPT_K, OPT_T)
        try:
            eng.setSeed(SEED)
            eps = nln_noise(SEED, 0, OPT_K, OPT_T, 1, cfg["std_dev"])[None]
            eng.computeControl(cfg["x0"], 1)
            orc.vanilla_compute_control(cfg["x0"], 1, eps)
            info = eng.getLaunchInfo()
            assert info["rows_in_hbm"] and info["family"] == case["expect"]["family"], info
            _assert_parity(eng, orc, "vanilla", "rows in HBM, " + case["id"])
        finally:
            eng.close()


# ------------------------------------------------------------------ 4: GPU, injected noise -----------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", [PARITY_CASES[1], PARITY_CASES[2], PARITY_CASES[10]], ids=lambda c: c["id"])
def test_injected_noise_is_taken_as_the_nln_noise_itself(gpu, case):
    """the same injected eps through an NLN handle and a Gaussian handle: bit-identical costs and u* (the buffer is eps', it
    is not multiplied by a log-normal factor again) — row pre-fill, in-loop draw and Robust MPPI's sampleAt"""
    K, T = 333, 9
    got = []
    for sampler in (NLN, m.MPPI_SAMPLER_GAUSSIAN):
        cfg, eng, _, _ = _make(case, K, T, sampler=sampler)
        try:
            C, S = eng.CONTROL_DIM, eng.STATE_DIM
            assert eng.sampler == sampler
            eng.injectNoise(host_noise(1, K, T, C, seed=7))
            if case["controller"] == "robust":
                eng.updateImportanceSamplingControl(cfg["x0"], 1)
                eng.setFeedbackGains(np.random.default_rng(5).uniform(-0.3, 0.3, (T, S, C)).astype(np.float32))
                eng.computeControl(cfg["x0"], 1)
                eng.updateImportanceSamplingControl(cfg["x0"], 1)  # the candidate evaluation: sampleAt on the buffer
            eng.computeControl(cfg["x0"], 1)
            assert eng.getLaunchInfo()["family"] == case["expect"]["family"]
            got.append((eng.getSampledCostSeq().copy(), eng.getControlSeq().copy(), eng.getSampledControls().copy()))
        finally:
            eng.close()
    for a, b in zip(*got):
        assert np.isfinite(a).all() and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ 5: GPU, moments of the dumped samples ---------------
@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(block_x=64, block_y=1, kernel_variant=P), dict(block_x=64, block_y=4, kernel_variant=F)],
                         ids=["in-loop-draw", "row-pre-fill"])
def test_nln_moments_of_the_dumped_samples(gpu, kw):
    """shares no code with the engine's draw or the oracle: e = (v - mu) / sigma of the dumped samples has the analytic second
    moment exp(2 sigma^2) of z * exp(sigma z') and mean 0, each within 4 standard errors.  Optimisation stride 0, so every
    step of rollouts k >= 1 holds noise (t < stride would take the mean)."""
    K, T, s = 4096, 8, 0.5
    cfg = cartpole_cfg(K=K, T=T, soft=True)
    cfg.update(std_dev=[s], pure_pct=0.0, ranges=[[-1e6, 1e6]])
    eng = make_engine(cfg, save_samples=True, sampler=NLN, **kw)
    try:
        for g in range(2):
            mu = eng.getOptimalControlSeq().astype(np.float64).reshape(1, T, 1)
            eng.computeControl(cfg["x0"], 0)
            v = eng.getSampledControls().astype(np.float64).reshape(K, T, 1)
            e = (v[1:] - mu) / np.float64(np.float32(s))
            n = e.size
            assert n == (K - 1) * T
            m2, m1 = float((e * e).mean()), float(e.mean())
            want = np.exp(2 * s * s)
            b2 = 4 * np.sqrt((3 * np.exp(8 * s * s) - np.exp(4 * s * s)) / n)
            b1 = 4 * np.sqrt(np.exp(2 * s * s) / n)
            print("generation %d: mean(e^2) = %.5f (analytic %.5f, bound %.5f), mean(e) = %.5f (bound %.5f)" % (
                g, m2, want, b2, m1, b1))
            assert abs(m2 - want) <= b2, (g, m2, want, b2)
            assert abs(m1) <= b1, (g, m1, b1)
    finally:
        eng.close()


# ------------------------------------------------------------------ 6: GPU, refusals -----------------------------------
@pytest.mark.gpu
def test_nln_refusals(gpu):
    with pytest.raises(m.MPPIError) as e:
        m.VanillaMPPIController("cartpole", 128, 8, 0.02, 1.0, sampler=NLN, noise_source=MPPI_NOISE_ROCRAND_HOST)
    assert e.value.status == m.MPPI_ERR_UNSUPPORTED and "NLN" in str(e.value), (e.value.status, str(e.value))
    with pytest.raises(m.MPPIError) as e:
        m.ColoredMPPIController("cartpole", 128, 8, 0.02, 1.0, sampler=NLN)
    assert e.value.status == m.MPPI_ERR_INVALID_ARG, e.value.status
    with pytest.raises(m.MPPIError) as e:
        m.VanillaMPPIController("cartpole", 128, 8, 0.02, 1.0, sampler=m.MPPI_SAMPLER_COLORED)
    assert e.value.status == m.MPPI_ERR_INVALID_ARG, e.value.status
    with pytest.raises(m.MPPIError) as e:
        m.VanillaMPPIController("racer_dubins", 128, 8, 0.02, 1.0, sampler=NLN)
    assert e.value.status == m.MPPI_ERR_UNKNOWN_MODEL, e.value.status
    # an NLN handle is no colored-noise handle; the Gaussian setters work on it
    eng = m.VanillaMPPIController("cartpole", 128, 8, 0.02, 1.0, sampler=NLN)
    try:
        with pytest.raises(m.MPPIError):
            eng._check(eng._lib.mppi_set_colored_noise_params(eng._h, np.zeros(1, np.float32), 0.97, 0.0))
        eng.setSamplingParams([0.5], [0.0], 0.01, 1.0)
        eng.setIndependentNoise(False)
        eng.setTimeSpecificStdDev(np.full((8, 1), 0.5, np.float32))
    finally:
        eng.close()
    # mppi_create is mppi_create_with_sampler(GAUSSIAN) for a Vanilla controller
    eng = m.VanillaMPPIController("cartpole", 128, 8, 0.02, 1.0)
    try:
        assert eng.sampler == m.MPPI_SAMPLER_GAUSSIAN
    finally:
        eng.close()


# ------------------------------------------------------------------ 7: GPU, sharding -----------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", [PARITY_CASES[1], PARITY_CASES[2]], ids=lambda c: c["id"])
def test_nln_draw_uses_the_global_rollout_index_when_k_is_sharded(gpu, case):
    """K = 200 over 2 in-process ranks, the exchange driven by the caller (tests/test_sharded_matrix.py): every rank's costs and
    clamped samples 0 ulp from the un-sharded oracle's slice, u* within 1e-5 of the oracle's un-sharded iteration"""
    K, W, T = 200, 2, 9
    Kl = K // W
    ranks, orc, cfg = [], None, None
    try:
        for r in range(W):
            cfg, eng, o, _ = _make(dict(case, kw=dict(case["kw"], rank=r, world_size=W)), K, T)
            ranks.append(eng)
            orc = orc or o
        x0 = cfg["x0"][None]
        for e in ranks:
            e.setSeed(SEED)
            e.uploadState(x0)
        mean = ranks[0].getOptimalControlSeq()
        eps = nln_noise(SEED, 0, K, T, 1, cfg["std_dev"])
        send = []
        for e in ranks:
            e.iterationLocal()
            send.append(e.readSendRecord())
        gathered = np.concatenate(send)
        for e in ranks:
            e.writeRecvRecords(gathered)
            e.iterationMerge()
        v_o = orc.set_gaussian_controls(mean, eps, 1, 0)
        costs_o, v_o = orc.rollout_costs(x0, mean, v_o)
        want = orc.iterate(x0, np.zeros((1, T, 1), np.float32), eps, 1, 0)
        for r, e in enumerate(ranks):
            sl = slice(r * Kl, (r + 1) * Kl)
            assert e.getLaunchInfo()["family"] == case["expect"]["family"]
            assert int(ulp_diff(e.getSampledCostSeq(), costs_o[:, sl]).max()) == 0, "rank %d costs" % r
            assert int(ulp_diff(e.getSampledControls(), v_o[:, sl]).max()) == 0, "rank %d samples" % r
            assert float(np.abs(e.getOptimalControlSeq() - want).max()) <= U_TOL, "rank %d u*" % r
    finally:
        for e in ranks:
            e.close()
