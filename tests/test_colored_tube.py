"""Tube-MPPI with the colored-noise sampler (the reference's TubeMPPIController<..., ColoredNoiseDistribution<...>>): one colored
draw per rollout written into the rows of both systems by the prologue GEMM, then the existing two-system code.

The reference answer is composed, the oracle is unchanged:
    eps[i] = pyoracle.colored_noise(z[i], exponents, offset_decay_rate, fmin, offset_t=stride, flavour="gemm")
    Oracle(model, K, T, D=2).tube_compute_control(x, stride, eps)
flavour "gemm" is the one tests/test_colored_noise.py holds the one-system Colored handle to, bit for bit: the engine's own
arithmetic, radix-4 butterfly + quarter-size GEMM where T is a multiple of 4 and at least 16, the dense table otherwise.  (T = 8
and T = 6 are both on the dense path; the T = 16 cases below are the radix-4 ones, with its per-system offset pass.)

The bars are the project's, not this code's: trajectory costs equal to the oracle's bit for bit (tests/test_colored_noise.py:
test_colored_rollout_costs_bit_exact), control sequences within 1e-5 (common.U_TOL), trajectories within 1e-4 and baselines to
1e-5 relative (tests/test_gpu_parity.py: test_tube_double_integrator_parity).

Shapes: K = 80 is one full block of 64 rollouts plus a partial block of 16, K = 16 a single partial block; every case runs in
well under a second.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mppi_generic_amd as m
import native_build as nb
import pyoracle as po
from common import SEED, U_TOL, cartpole_cfg_lr, colored_cartpole, di_cfg, host_noise, host_spectrum, make_engine, make_oracle, ulp_diff
from kernel_forms import env_override

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLORED = m.MPPI_SAMPLER_COLORED
MODELS = ("double_integrator", "cartpole")
DRIFT = {"double_integrator": np.array([0.05, -0.03, 0.2, -0.1], np.float32), "cartpole": np.array([0.2, -0.4, 0.1, 0.5], np.float32)}


def tube_cfg(model, K, T, num_iters=1, decay=1.0):
    if model == "double_integrator":
        cfg = di_cfg(K=K, T=T, tube=True, num_iters=num_iters)
        cfg["colored"] = ([1.0, 0.5], 0.97, 0.0)
    else:  # likelihood-ratio cost, terminal cost, alpha, control limits; its own exploration for each system
        cfg = cartpole_cfg_lr(K=K, T=T)
        cfg["D"] = 2
        cfg["num_iters"] = num_iters
        cfg["std_dev"] = [5.0, 4.0]
        cfg["colored"] = ([1.0], 0.97, 0.0)
    cfg["decay"] = decay
    return cfg


def make_tube_colored(cfg, **kw):
    c = m.TubeMPPIController(cfg["model"], cfg["K"], cfg["T"], cfg["dt"], cfg["lambda_"], cfg["alpha"], cfg["num_iters"], seed=SEED,
                             sampler=COLORED, **kw)
    if cfg["dyn"] is not None:
        c.setDynamicsParams(cfg["dyn"])
    c.setCostParams(cfg["cost"])
    if cfg["ranges"] is not None:
        c.setControlRanges(cfg["ranges"])
    c.setSamplingParams(cfg["std_dev"], cfg["control_cost_coeff"], cfg.get("pure_pct", 0.01), cfg.get("decay", 1.0))
    c.setColoredNoiseParams(*cfg["colored"])
    return c


def colored_eps(cfg, z, stride):
    """z [n][K][C][T+1][2] -> eps [n][K][T][C], the one draw both systems see"""
    exps, decay, fmin = cfg["colored"]
    return np.stack([po.colored_noise(zi, exps, decay, fmin, stride, flavour="gemm") for zi in z])


def test_creation_and_launch_shape(gpu):
    """the creation the parent commit refused with MPPI_ERR_INVALID_ARG: D = 2, the colored sampler, the fused kernel on (64, 1, 2)"""
    for model in MODELS:
        eng = make_tube_colored(tube_cfg(model, 80, 8))
        assert eng.num_systems == 2 and eng.sampler == COLORED
        eng.computeControl(tube_cfg(model, 80, 8)["x0"], 1)
        info = eng.getLaunchInfo()
        assert info["family"] == "fused" and info["block"] == (64, 1, 2) and not info["rows_in_hbm"], info
        eng.close()
        eng = make_tube_colored(tube_cfg(model, 80, 8), kernel_variant=m.MPPI_KERNEL_FUSED, block_x=64, block_y=1)
        eng.close()
    # mppi_create alone keeps Tube on the Gaussian sampler
    eng = make_engine(di_cfg(K=80, T=8, tube=True))
    assert eng.sampler == m.MPPI_SAMPLER_GAUSSIAN
    eng.close()


def test_refusals(gpu):
    cfg = tube_cfg("double_integrator", 80, 8)
    with pytest.raises(m.MPPIError) as e:
        make_tube_colored(cfg, kernel_variant=m.MPPI_KERNEL_PIPELINE)
    assert e.value.status == m.MPPI_ERR_LAUNCH_SHAPE and "no form for the Tube controller with MPPI_SAMPLER_COLORED" in str(e.value)
    with pytest.raises(m.MPPIError) as e:
        make_tube_colored(cfg, block_x=32, block_y=1)  # the fold's shape
    assert e.value.status == m.MPPI_ERR_LAUNCH_SHAPE
    with pytest.raises(m.MPPIError) as e:
        m.RobustMPPIController("double_integrator", 80, 8, 0.02, 1.0, sampler=COLORED)
    assert e.value.status == m.MPPI_ERR_UNSUPPORTED and "random access" in str(e.value)
    with pytest.raises(m.MPPIError) as e:
        m.VanillaMPPIController("double_integrator", 80, 8, 0.02, 1.0, sampler=COLORED)
    assert e.value.status == m.MPPI_ERR_INVALID_ARG
    eng = make_tube_colored(cfg)
    with pytest.raises(m.MPPIError) as e:
        eng.setIndependentNoise(True)
    assert e.value.status == m.MPPI_ERR_UNSUPPORTED and "no per-system spectrum stream is assigned" in str(e.value)
    with pytest.raises(m.MPPIError) as e:  # Tsallis weights and the leash stay with MPPI_CONTROLLER_COLORED
        eng._check(eng._lib.mppi_set_colored_mppi_params(eng._h, 1.0, 2.0, None, 0, 1))
    assert e.value.status == m.MPPI_ERR_STATE
    # the refusals left the handle as it was: shared noise, and it computes
    eng.setIndependentNoise(False)
    eng.computeControl(cfg["x0"], 1)
    assert np.isfinite(eng.getControlSeq()).all()
    eng.close()


# K, T, stride, num_iters, std_dev_decay
CASES = [(80, 8, 1, 1, 1.0), (80, 6, 1, 1, 1.0), (16, 8, 1, 1, 1.0), (16, 6, 1, 1, 1.0), (80, 8, 2, 2, 0.9),
         (80, 16, 1, 1, 1.0), (16, 16, 2, 2, 0.9)]


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("K,T,stride,num_iters,decay", CASES, ids=["K%d-T%d-s%d-i%d" % c[:4] for c in CASES])
def test_rollout_costs_bit_exact_with_different_initial_states(gpu, model, K, T, stride, num_iters, decay):
    """one launch, injected spectrum, a non-zero mean, and the two systems started from DIFFERENT states: a row written to the
    wrong system, a missed offset pass of the partial block, or a wrong sigma per system shows in the costs [2][K]"""
    cfg = tube_cfg(model, K, T, num_iters, decay)
    eng, orc = make_tube_colored(cfg), make_oracle(cfg)
    Cd = eng.CONTROL_DIM
    z = host_spectrum(1, K, T, Cd, seed=3)
    mean = (0.2 * np.sin(np.arange(T * Cd, dtype=np.float32) * 0.3)).reshape(T, Cd)
    x0 = np.stack([cfg["x0"], cfg["x0"] + DRIFT[model]])
    eng.updateImportanceSampler(mean)
    eng.injectNoise(z)
    got = eng.rolloutCosts(x0, stride)
    mean2 = np.stack([mean, mean])
    v = orc.set_gaussian_controls(mean2, colored_eps(cfg, z, stride)[0], stride, 0)
    want, _ = orc.rollout_costs(x0, mean2, v)
    assert got.shape == (2, K) and np.isfinite(got).all()
    assert not np.array_equal(want[0], want[1])
    assert ulp_diff(got, want).max() == 0
    eng.close()


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("K,T,stride,num_iters,decay", CASES, ids=["K%d-T%d-s%d-i%d" % c[:4] for c in CASES])
def test_compute_control_parity(gpu, model, K, T, stride, num_iters, decay):
    """three calls of the Tube loop with the measured state pushed away from the nominal one in between: costs (bit for bit while
    both sides start from the same mean: the first call of a one-iteration handle), both control sequences, both state
    trajectories, the statistics and nominal_state_used"""
    cfg = tube_cfg(model, K, T, num_iters, decay)
    eng, orc = make_tube_colored(cfg), make_oracle(cfg)
    Cd = eng.CONTROL_DIM
    x = cfg["x0"].copy()
    for i in range(3):
        z = host_spectrum(num_iters, K, T, Cd, seed=20 + i)
        eng.injectNoise(z)
        eng.computeControl(x, stride)
        orc.tube_compute_control(x, stride, colored_eps(cfg, z, stride))
        costs = eng.getSampledCostSeq()
        du = float(np.abs(eng.getControlSeq() - orc.control()).max())
        dn = float(np.abs(eng.getNominalControlSeq() - orc.nominal_control()).max())
        st, so = eng.getStats(), orc.stats()
        print("%s K=%d T=%d call %d: cost ulp %d, u %.3g, u_nominal %.3g" % (model, K, T, i, int(ulp_diff(costs, orc.costs()).max()), du, dn))
        if i == 0 and num_iters == 1:
            assert ulp_diff(costs, orc.costs()).max() == 0
        assert du <= U_TOL and dn <= U_TOL
        assert np.abs(eng.getTargetStateSeq() - orc.state_traj()).max() <= 1e-4
        assert np.abs(eng.getNominalStateSeq() - orc.nominal_state_traj()).max() <= 1e-4
        assert abs(st.real_sys.baseline - so["baseline"][0]) <= 1e-5 * abs(so["baseline"][0])
        assert abs(st.nominal_sys.baseline - so["baseline"][1]) <= 1e-5 * abs(so["baseline"][1])
        assert abs(st.real_sys.normalizer - so["normalizer"][0]) <= 1e-5 * so["normalizer"][0]
        assert abs(st.nominal_sys.normalizer - so["normalizer"][1]) <= 1e-5 * so["normalizer"][1]
        assert st.nominal_state_used == so["nominal_state_used"]
        x = x + DRIFT[model] * (i + 1)
    eng.close()


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("T", [8, 16], ids=["dense", "radix4"])
def test_rows_in_hbm(gpu, model, T):
    """MPPI_AMD_ROWS_IN_HBM=1: the prologue writes the rows of both systems to the HBM buffer ([block][2 x 64 slots][row]), the
    step loop and the block softmin read them back; same costs bit for bit, same controls"""
    K = 80
    cfg = tube_cfg(model, K, T)
    with env_override(MPPI_AMD_ROWS_IN_HBM="1"):
        eng = make_tube_colored(cfg)
    orc = make_oracle(cfg)
    z = host_spectrum(1, K, T, eng.CONTROL_DIM, seed=5)
    eng.injectNoise(z)
    eng.computeControl(cfg["x0"], 1)
    info = eng.getLaunchInfo()
    assert info["family"] == "fused" and info["block"] == (64, 1, 2) and info["rows_in_hbm"], info
    orc.tube_compute_control(cfg["x0"], 1, colored_eps(cfg, z, 1))
    assert ulp_diff(eng.getSampledCostSeq(), orc.costs()).max() == 0
    assert np.abs(eng.getControlSeq() - orc.control()).max() <= U_TOL
    assert np.abs(eng.getNominalControlSeq() - orc.nominal_control()).max() <= U_TOL
    eng.close()


@pytest.mark.parametrize("model", MODELS)
def test_same_noise_gives_identical_cost_rows(gpu, model):
    """the reference's own check (tests/mppi_core/rollout_kernel_tests.cu:181-198): the same state for both systems gives
    bit-identical cost rows — with an injected spectrum and with the in-kernel Philox spectrum"""
    cfg = tube_cfg(model, 80, 16)
    cfg["std_dev"] = cfg["std_dev"][:1] if model == "cartpole" else cfg["std_dev"]  # one sigma for both systems
    eng = make_tube_colored(cfg)
    x2 = np.tile(cfg["x0"], (2, 1))
    eng.injectNoise(host_spectrum(1, 80, 16, eng.CONTROL_DIM, seed=8))
    costs = eng.rolloutCosts(x2, 1)
    assert np.isfinite(costs).all() and np.array_equal(costs[0], costs[1])
    eng.injectNoise(None)
    eng.setSeed(99)
    costs = eng.rolloutCosts(x2, 1)
    assert np.isfinite(costs).all() and np.array_equal(costs[0], costs[1]) and costs[0].std() > 0
    eng.close()


@pytest.mark.parametrize("T,stride", [(8, 1), (16, 2)])
def test_generator_path_equals_the_colored_controller(gpu, T, stride):
    """Philox noise: mppi_sample_noise of the Tube handle equals that of an MPPI_CONTROLLER_COLORED handle of the same seed, K, T
    and parameters bit for bit — and so does what the oracle makes of the Philox spectrum"""
    K = 80
    cfg = tube_cfg("double_integrator", K, T)
    tube = make_tube_colored(cfg)
    one = di_cfg(K=K, T=T, tube=False)
    one["colored"] = cfg["colored"]
    col = make_engine(one)
    assert col.sampler == COLORED and col.num_systems == 1
    for eng in (tube, col):
        eng.setSeed(1234)
    a, b = tube.sampleNoise(stride), col.sampleNoise(stride)
    assert np.array_equal(a.view(np.int32), b.view(np.int32))
    exps, decay, fmin = cfg["colored"]
    zp = po.philox_spectrum(1234, 0, K, T, 2)
    assert ulp_diff(a, po.colored_noise(zp, exps, decay, fmin, stride, flavour="gemm")).max() == 0
    # ... and the rollouts draw that spectrum: the Philox run equals the run with the same spectrum injected
    tube.computeControl(cfg["x0"], stride)
    u, un, c = tube.getControlSeq(), tube.getNominalControlSeq(), tube.getSampledCostSeq()
    again = make_tube_colored(cfg)
    again.injectNoise(zp[None])
    again.computeControl(cfg["x0"], stride)
    assert np.array_equal(c, again.getSampledCostSeq())
    assert np.array_equal(u, again.getControlSeq()) and np.array_equal(un, again.getNominalControlSeq())
    for eng in (tube, col, again):
        eng.close()


def test_reference_order_reduction_as_for_a_gaussian_tube_handle(gpu):
    """MPPI_REDUCTION_REFERENCE_ORDER works downstream of the rows, whatever filled them: same bar against the oracle"""
    cfg = tube_cfg("double_integrator", 80, 8)
    eng, orc = make_tube_colored(cfg), make_oracle(cfg)
    eng.setReductionMode(m.MPPI_REDUCTION_REFERENCE_ORDER)
    z = host_spectrum(1, 80, 8, 2, seed=31)
    eng.injectNoise(z)
    eng.computeControl(cfg["x0"], 1)
    orc.tube_compute_control(cfg["x0"], 1, colored_eps(cfg, z, 1))
    assert np.abs(eng.getControlSeq() - orc.control()).max() <= U_TOL
    assert np.abs(eng.getNominalControlSeq() - orc.nominal_control()).max() <= U_TOL
    eng.close()


def test_other_handles_of_the_process_are_not_disturbed(gpu):
    """a Gaussian Tube handle and a Colored (one-system) handle give, next to a Tube handle with colored noise that runs in
    between, what they give alone — bit for bit"""
    K, T = 80, 16
    gcfg = di_cfg(K=K, T=T, tube=True)
    ccfg = colored_cartpole(K=K, T=T)
    eps = host_noise(1, K, T, 2, seed=4)
    zc = host_spectrum(1, K, T, 1, seed=6)

    def run_gaussian(eng):
        eng.injectNoise(eps)
        eng.computeControl(gcfg["x0"], 1)
        return eng.getControlSeq(), eng.getNominalControlSeq(), eng.getSampledCostSeq()

    def run_colored(eng):
        eng.injectNoise(zc)
        eng.computeControl(ccfg["x0"], 1)
        return eng.getControlSeq(), eng.getSampledCostSeq()

    g, c = make_engine(gcfg), make_engine(ccfg)
    alone_g, alone_c = run_gaussian(g), run_colored(c)
    g.close()
    c.close()
    tcfg = tube_cfg("cartpole", K, T)
    tc, g, c = make_tube_colored(tcfg), make_engine(gcfg), make_engine(ccfg)
    tc.injectNoise(host_spectrum(1, K, T, 1, seed=7))
    tc.computeControl(tcfg["x0"], 1)
    with_g = run_gaussian(g)
    tc.computeControl(tcfg["x0"], 1)
    with_c = run_colored(c)
    tc.computeControl(tcfg["x0"], 1)
    assert all(np.array_equal(a, b) for a, b in zip(alone_g, with_g))
    assert all(np.array_equal(a, b) for a, b in zip(alone_c, with_c))
    assert g.getLaunchInfo()["family"] == "pipeline_fold" and c.getLaunchInfo()["family"] == "pipeline"
    for eng in (tc, g, c):
        eng.close()


# ------------------------------------------------------------------ the templated host surface --------------------------
NAME = "templated_double_integrator_colored_tube"


def _build_example():
    return nb.build_example(m, NAME, "-I" + os.path.join(REPO, "examples"))


def test_templated_example_prints_the_sums_python_gets(gpu):
    """TubeMPPIController<DoubleIntegratorDynamics, DoubleIntegratorCircleCost, DDPFeedback, 48, 1024, ColoredNoiseDistribution<...>>
    from the reference's include paths: builds, runs the fused (64, 1, 2) kernel of ITS translation unit, and after the same four
    control steps its two control sequences sum to what the name-keyed controller's do (1e-5 per element, 96 elements)"""
    txt = open(os.path.join(REPO, "examples", NAME + ".hip")).read()
    incs = re.findall(r'#include [<"]([^>"]+)[>"]', txt)
    assert "mppi/sampling_distributions/colored_noise/colored_noise.cuh" in incs
    assert all(i.startswith("mppi/") or "/" not in i for i in incs), incs
    exe = _build_example()
    blob = open(exe, "rb").read()
    assert re.search(rb"rolloutKernel[A-Za-z0-9_]*ColoredNoiseDistribution[A-Za-z0-9_]*Li64ELi1ELi2E", blob) and b"gfx950" in blob
    steps, K, T = 4, 1024, 48
    r = subprocess.run([exe, str(steps)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Tube MPPI with colored noise: %d control steps" % steps in r.stdout, r.stdout[-500:]
    su = float(re.search(r"^sum u = (\S+)$", r.stdout, flags=re.M).group(1))
    sn = float(re.search(r"^sum u_nominal = (\S+)$", r.stdout, flags=re.M).group(1))
    cfg = di_cfg(K=K, T=T, tube=True)
    cfg["colored"] = ([1.0, 0.5], 0.97, 0.0)
    eng = make_tube_colored(cfg)
    eng.setNominalThreshold(20.0)
    x = np.array([2.0, 0.0, 0.0, 1.0], np.float32)
    for i in range(steps):
        eng.computeControl(x, 1)
        x = x + np.array([0.01, 0.0, 0.02, 0.0], np.float32)
        if i + 1 < steps:
            eng.slideControlSequence(1)
    pu = float(eng.getControlSeq().astype(np.float64).sum())
    pn = float(eng.getNominalControlSeq().astype(np.float64).sum())
    eng.close()
    print("templated colored Tube: sum u %.9g (python %.9g), sum u_nominal %.9g (python %.9g)" % (su, pu, sn, pn))
    assert abs(su) > 1e-3 and abs(su - pu) <= 96 * U_TOL and abs(sn - pn) <= 96 * U_TOL


MPPI_NOISE_ROCRAND_HOST = 2


def test_rocrand_host_fills_the_one_spectrum_as_for_a_colored_handle(gpu):
    """MPPI_NOISE_ROCRAND_HOST: the host generator fills z[K][C][T+1][2] once per launch, whatever the controller — the Tube
    handle's system 0 samples what an MPPI_CONTROLLER_COLORED handle of the same seed, K, T and parameters samples (same stretch
    of the rocRAND stream, same transform, both from a zero mean), bit for bit; and both systems see that one draw"""
    K, T = 80, 16
    cfg = tube_cfg("double_integrator", K, T)
    tube = make_tube_colored(cfg, noise_source=MPPI_NOISE_ROCRAND_HOST, save_samples=True)
    one = di_cfg(K=K, T=T, tube=False)
    one["colored"] = cfg["colored"]
    col = make_engine(one, noise_source=MPPI_NOISE_ROCRAND_HOST, save_samples=True)
    assert col.sampler == COLORED and col.num_systems == 1
    x2 = np.tile(cfg["x0"], (2, 1))
    costs = tube.rolloutCosts(x2, 1)
    assert np.isfinite(costs).all() and np.array_equal(costs[0], costs[1]) and costs[0].std() > 0
    v = tube.getSampledControls()
    assert np.array_equal(v[0], v[1])
    col.rolloutCosts(cfg["x0"][None], 1)
    assert np.array_equal(v[0].view(np.int32), col.getSampledControls()[0].view(np.int32))
    # the next launch draws the next stretch of the stream, and the loop runs
    tube.computeControl(cfg["x0"], 1)
    assert not np.array_equal(tube.getSampledControls()[0][1:], v[0][1:])
    assert np.isfinite(tube.getControlSeq()).all() and np.isfinite(tube.getNominalControlSeq()).all()
    for eng in (tube, col):
        eng.close()


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("T,philox", [(16, False), (6, False), (16, True)], ids=["radix4", "dense", "philox"])
def test_two_ranks_against_the_unsharded_oracle(gpu, model, T, philox):
    """K = 160 over two ranks (each one full block and a partial one), both handles in this process, the exchange staged through
    the host as in tests/test_sharded_matrix.py: every rank's costs and clamped samples 0 ulp from the un-sharded oracle's slice
    (the spectrum is indexed by the global rollout), u* of both systems within 1e-5 of the oracle's un-sharded iteration and
    bit-identical on the two ranks"""
    K, W, seed = 160, 2, 77
    Kl = K // W
    cfg = tube_cfg(model, K, T)
    orc = make_oracle(cfg)
    ranks = [make_tube_colored(cfg, rank=r, world_size=W, save_samples=True) for r in range(W)]
    try:
        Cd = ranks[0].CONTROL_DIM
        for r, e in enumerate(ranks):
            assert (e.num_rollouts_local, e.rollout_offset) == (Kl, r * Kl)
        if philox:
            z = po.philox_spectrum(seed, 0, K, T, Cd)
            for e in ranks:
                e.setSeed(seed)
        else:
            z = host_spectrum(1, K, T, Cd, seed=K + T)[0]
            for r, e in enumerate(ranks):
                e.injectNoise(np.ascontiguousarray(z[r * Kl:(r + 1) * Kl])[None])
        eps = colored_eps(cfg, z[None], 1)[0]
        x0 = np.stack([cfg["x0"], cfg["x0"] + DRIFT[model]])
        send = []
        for e in ranks:
            e.uploadState(x0)
        mean = ranks[0].getOptimalControlSeq()
        for e in ranks:
            e.iterationLocal()
            send.append(e.readSendRecord())
        for e in ranks:
            e.writeRecvRecords(np.concatenate(send))
            e.iterationMerge()
        v_o = orc.set_gaussian_controls(mean, eps, 1, 0)
        costs_o, v_o = orc.rollout_costs(x0, mean, v_o)
        for r, e in enumerate(ranks):
            info = e.getLaunchInfo()
            assert info["family"] == "fused" and info["block"] == (64, 1, 2), info
            sl = slice(r * Kl, (r + 1) * Kl)
            assert ulp_diff(e.getSampledCostSeq(), costs_o[:, sl]).max() == 0, "rank %d" % r
            assert ulp_diff(e.getSampledControls(), v_o[:, sl]).max() == 0, "rank %d" % r
        want = orc.iterate(x0, np.zeros_like(mean), eps, 1, 0)
        us = [e.getOptimalControlSeq() for e in ranks]
        assert np.array_equal(us[0].view(np.int32), us[1].view(np.int32))
        assert np.abs(us[0] - want).max() <= U_TOL
    finally:
        for e in ranks:
            e.close()
