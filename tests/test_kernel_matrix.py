"""Every registered rollout kernel instantiation against the oracle at edge shapes, enumerated from the registry.

The cases come from mppi_list_models + mppi_describe_model, not from a hand-written list: one case per reachable
(registration, controller, requested kernel form).  A registration without a configuration builder fails the CPU test
below, so a new model cannot skip parity.  Every case runs a short fixed list of (K, T) — one rollout, partial waves and
blocks, a ragged K >= 1000, horizons shorter than a sampler trip or a pair of steps, and for colored noise the radix-4
edges T = 16, 17 — and asserts
  - mppi_get_launch_info == the form the case asked for (an intended fallback is written into the case as its expectation);
  - injected noise: sampled costs 0 ulp against the oracle, u* within 1e-5 (both systems for Tube / Robust);
  - once per case, the in-kernel Philox stream: the same against po.philox_normal / po.philox_spectrum;
  - where u* is a softmin of the handle's own rollouts (Vanilla, Colored, Tube): u* == sum_k w_k v_k / sum_k w_k in float64
    from the engine's own dumped costs and samples, within 2e-6 max(1, |u|) — a check that shares no code with the
    engine (the oracle mirrors det_math.h and the engine's reduction order, so it cannot see a reduction bug both share).
A controller that refuses a requested form is asserted to refuse it with the documented status.
"""
import os

import numpy as np
import pytest

import mppi_generic_amd as m
import pyoracle as po
from common import (autorally_cfg, bicycle_lstm_cfg, cartpole_cfg_lr, di_cfg, host_noise, host_spectrum, make_engine,
                    make_oracle, racer_cfg, ulp_diff)

U_TOL = 1e-5
SOFTMIN_RTOL = 2e-6
MPPI_ERR_INVALID_ARG = 1
MPPI_ERR_LAUNCH_SHAPE = 5


def _racer(mk_name):
    def build(K, T, D):
        if mk_name == "elevation":
            from test_racer_dubins_elevation import elevation_cfg as mk
        elif mk_name == "steering":
            from test_racer_dubins_lstm_steering import steering_cfg as mk
        elif mk_name == "uncertainty":
            from test_racer_dubins_lstm_unc import uncertainty_cfg as mk
        else:
            from test_racer_dubins_suspension import suspension_cfg as mk
        return mk(K=K, T=T, D=D)
    return build


def _plain(mk, **kw):
    def build(K, T, D):
        cfg = mk(K=K, T=T, **kw)
        cfg["D"] = D
        return cfg
    return build


def _di_robust_cost(K, T, D):
    from test_double_integrator_robust_cost import robust_cfg
    return robust_cfg(K=K, T=T, tube=D == 2)


# configuration builder per registered model name: (K, T, systems) -> the cfg dict of common.py
BUILDERS = {
    "cartpole": _plain(cartpole_cfg_lr),
    "double_integrator": lambda K, T, D: di_cfg(K=K, T=T, tube=D == 2),
    "double_integrator_robust": _di_robust_cost,
    "racer_dubins": _plain(racer_cfg),
    "autorally_nn": _plain(autorally_cfg),
    "bicycle_slip_lstm": _plain(bicycle_lstm_cfg),
    "racer_dubins_elevation": _racer("elevation"),
    "racer_dubins_elevation_lstm_steering": _racer("steering"),
    "racer_dubins_elevation_lstm_unc": _racer("uncertainty"),
    "racer_dubins_elevation_suspension": _racer("suspension"),
}

KT = [(1, 1), (63, 2), (65, 3), (200, 5), (1049, 9)]
KT_COLORED = KT + [(65, 16), (200, 17)]
PHILOX_KT = (65, 5)


def _registrations():
    out = []
    for name in m.list_models():
        for sampler in (m.MPPI_SAMPLER_GAUSSIAN, m.MPPI_SAMPLER_COLORED):
            d = m.describe_model(name, sampler)
            if d is not None:
                out.append((name, sampler, d))
    return out


def _pipeline_family(d, shape):
    """the role-pipelined kernel mppi_create runs for a shape (mppi_create's pipe_ok), or None"""
    bx, by, bz = shape
    if shape in d["replicated_lane_shapes"]:
        return "pipeline_rep" if (bx == 64 and bz == 1) else None
    if d["pipeline_fold"] and shape == (32, 1, 2):
        return "pipeline_fold"
    if d["pipeline"] and bx == 64 and by == 1:
        return "pipeline"
    return None


def _case(reg, controller, form, kw, expect, hbm=False, refuse=None):
    name, sampler, _ = reg
    tag = "%s%s-%s-%s%s" % (name, "[colored]" if sampler else "", controller, form, "-hbm" if hbm else "")
    return dict(id=tag, model=name, controller=controller, kw=kw, expect=expect, hbm=hbm, refuse=refuse)


def build_cases():
    cases = []
    for reg in _registrations():
        name, sampler, d = reg
        fused_family = lambda s: "fused_rep" if s in d["replicated_lane_shapes"] else "fused"
        controllers = ["colored"] if sampler == m.MPPI_SAMPLER_COLORED else ["vanilla", "tube"] + (["robust"] if d["rmppi"] else [])
        for ctl in controllers:
            bz = 2 if ctl == "tube" else 1
            shapes = [s for s in d["shapes"] if s[2] == bz] if ctl != "robust" else []
            for s in shapes:
                kw = dict(block_x=s[0], block_y=s[1])
                cases.append(_case(reg, ctl, "fused%dx%dx%d" % s, dict(kw, kernel_variant=m.MPPI_KERNEL_FUSED),
                                   dict(family=fused_family(s), block=s, rows_in_hbm=False)))
                pf = _pipeline_family(d, s)
                if pf:
                    cases.append(_case(reg, ctl, "pipeline%dx%dx%d" % s, dict(kw, kernel_variant=m.MPPI_KERNEL_PIPELINE),
                                       dict(family=pf, block=s, rows_in_hbm=False)))
            if ctl == "tube" and d["pipeline_fold"]:
                # no shape requested: mppi_create folds the two systems into the lanes of a wave
                cases.append(_case(reg, ctl, "auto-fold", dict(kernel_variant=m.MPPI_KERNEL_AUTO),
                                   dict(family="pipeline_fold", block=(32, 1, 2), rows_in_hbm=False)))
            if ctl != "robust" and shapes and d["rows_in_hbm"]:
                # MPPI_AMD_ROWS_IN_HBM=1: the sample rows in HBM at any horizon, on the first registered shape of each kind
                first = shapes[0]
                cases.append(_case(reg, ctl, "fused%dx%dx%d" % first,
                                   dict(block_x=first[0], block_y=first[1], kernel_variant=m.MPPI_KERNEL_FUSED),
                                   dict(family=fused_family(first), block=first, rows_in_hbm=True), hbm=True))
                piped = [s for s in shapes if _pipeline_family(d, s)]
                if piped:
                    s = piped[0]
                    cases.append(_case(reg, ctl, "pipeline%dx%dx%d" % s,
                                       dict(block_x=s[0], block_y=s[1], kernel_variant=m.MPPI_KERNEL_PIPELINE),
                                       dict(family=_pipeline_family(d, s), block=s, rows_in_hbm=True), hbm=True))
            if ctl == "robust":
                for bx in (64, 32):
                    cases.append(_case(reg, ctl, "fused%dx1x2" % bx, dict(block_x=bx, kernel_variant=m.MPPI_KERNEL_FUSED),
                                       dict(family="rmppi", block=(bx, 1, 2), rows_in_hbm=False)))
                if d["rmppi_pipeline"]:
                    # the role-pipelined Robust kernel keeps its sample rows in HBM by design (the rings take the LDS)
                    cases.append(_case(reg, ctl, "pipeline64x1x2", dict(kernel_variant=m.MPPI_KERNEL_PIPELINE),
                                       dict(family="rmppi_pipeline", block=(64, 1, 2), rows_in_hbm=True)))
                else:
                    cases.append(_case(reg, ctl, "pipeline-refused", dict(kernel_variant=m.MPPI_KERNEL_PIPELINE), None,
                                       refuse=MPPI_ERR_LAUNCH_SHAPE))
                cases.append(_case(reg, ctl, "16x1x2-refused", dict(block_x=16, kernel_variant=m.MPPI_KERNEL_FUSED), None,
                                   refuse=MPPI_ERR_LAUNCH_SHAPE))
            # a pipeline request on a shape that has no pipelined form is refused, never run as something else
            unpiped = [s for s in shapes if not _pipeline_family(d, s)]
            if unpiped:
                s = unpiped[0]
                cases.append(_case(reg, ctl, "pipeline%dx%dx%d-refused" % s,
                                   dict(block_x=s[0], block_y=s[1], kernel_variant=m.MPPI_KERNEL_PIPELINE), None,
                                   refuse=MPPI_ERR_LAUNCH_SHAPE))
    return cases


# ------------------------------------------------------------------ CPU ------------------------------------------------
def test_every_registration_has_a_builder_and_cases(lib):
    """fails when a registered model has no configuration builder here (a new model cannot skip parity), when a
    registration yields no case, or when mppi_describe_model disagrees with the registration's own listing"""
    regs = _registrations()
    names = {r[0] for r in regs}
    assert names == set(m.list_models())
    missing = sorted(names - set(BUILDERS))
    assert not missing, "registered models without a kernel-matrix configuration builder: %s" % missing
    cases = build_cases()
    for name, sampler, d in regs:
        assert d["shapes"], (name, sampler)
        assert set(d["replicated_lane_shapes"]) <= set(d["shapes"]), (name, sampler)
        prefix = name + ("[colored]" if sampler else "") + "-"
        mine = [c for c in cases if c["id"].startswith(prefix) and not c["refuse"]]
        assert mine, "registration %s has no runnable case" % prefix
    ids = [c["id"] for c in cases]
    assert len(ids) == len(set(ids))
    # a colored-noise controller always runs one system: the colored registrations list no two-system shape
    for name, sampler, d in regs:
        if sampler == m.MPPI_SAMPLER_COLORED:
            assert all(s[2] == 1 for s in d["shapes"]), (name, d["shapes"])
            assert not d["rmppi"], name


def test_describe_model_without_device_and_unknown_names(lib):
    d = m.describe_model("cartpole")
    assert (64, 1, 1) in d["shapes"] and d["pipeline"] and d["rmppi"] and d["rows_in_hbm"] and d["pipeline_fold"]
    assert d["replicated_lane_shapes"] == [] and d["streamed_merge"]
    a = m.describe_model("autorally_nn")
    assert a["replicated_lane_shapes"][:2] == [(64, 4, 1), (32, 4, 1)] and not a["pipeline"] and a["rmppi_pipeline"]
    c = m.describe_model("double_integrator", m.MPPI_SAMPLER_COLORED)
    assert c["shapes"] == [(64, 1, 1)] and c["pipeline"] and not c["streamed_merge"] and not c["rmppi"]
    assert m.describe_model("no_such_model") is None
    import ctypes as C
    assert lib.mppi_describe_model(b"cartpole", 7, None, 0, None, None) == 1  # MPPI_ERR_INVALID_ARG
    n = C.c_int()
    assert lib.mppi_describe_model(b"cartpole", 0, None, 0, C.byref(n), None) == 0 and n.value == len(d["shapes"])


# ------------------------------------------------------------------ GPU ------------------------------------------------
CASES = build_cases()


def _colored_params(C):
    return ([1.0, 0.5][:C], 0.97, 0.0)


def _make(case, K, T, num_iters=1, overlay=None):
    """overlay: cfg entries that replace the builder's (and the Robust coefficients below) — the sampler options of
    tests/test_sampler_options_matrix.py; None leaves the configuration every test here runs on"""
    D = 2 if case["controller"] in ("tube", "robust") else 1
    cfg = BUILDERS[case["model"]](K, T, D)
    cfg["D"] = D
    cfg["num_iters"] = num_iters
    if case["controller"] == "colored":
        cfg["colored"] = _colored_params(len(cfg["control_cost_coeff"]))
    old = os.environ.get("MPPI_AMD_ROWS_IN_HBM")
    os.environ["MPPI_AMD_ROWS_IN_HBM"] = "1" if case["hbm"] else "0"
    try:
        if case["controller"] == "robust":
            from test_rmppi import _make_pair
            cfg["control_cost_coeff"] = [0.2, 0.1][:len(cfg["control_cost_coeff"])]
            cfg.update(overlay or {})
            # 9 x 32 candidate rollouts as bench.py; fewer rollouts than that take the smallest candidate set (3, odd) that fits
            nc, ns = (9, 32) if K >= 9 * 32 else (3, K // 3)
            eng, orc, rob = _make_pair(cfg, nc=nc, ns=ns, save_samples=True, **case["kw"])
        else:
            cfg.update(overlay or {})
            eng, orc, rob = make_engine(cfg, tube=D == 2, save_samples=True, **case["kw"]), make_oracle(cfg), None
    finally:
        if old is None:
            del os.environ["MPPI_AMD_ROWS_IN_HBM"]
        else:
            os.environ["MPPI_AMD_ROWS_IN_HBM"] = old
    return cfg, eng, orc, rob


def _softmin64(costs, v, lambda_):
    c = costs.astype(np.float64)
    w = np.exp(-(c - c.min()) / lambda_)
    return (w[:, None, None] * v.astype(np.float64)).sum(0) / w.sum()


def _run(case, K, T, philox):
    """one (K, T) of a case; returns nothing, asserts with the case's name in every message"""
    tag = "%s K=%d T=%d%s" % (case["id"], K, T, " philox" if philox else "")
    if case["controller"] == "robust" and K < 3:
        # RobustMPPIController needs at least 3 candidates x 1 sample (robust_mppi_controller.cu: candidates odd, >= 3)
        with pytest.raises(m.MPPIError) as e:
            _make(case, K, T)
        assert e.value.status == MPPI_ERR_INVALID_ARG, "%s: refused with %d" % (tag, e.value.status)
        return
    cfg, eng, orc, rob = _make(case, K, T)
    try:
        C, ctl = eng.CONTROL_DIM, case["controller"]
        if ctl == "colored":
            exps, decay, fmin = cfg["colored"]
            if philox:
                eng.setSeed(77)
                z = po.philox_spectrum(77, 0, K, T, C)[None]
            else:
                z = host_spectrum(1, K, T, C, seed=K + T)
                eng.injectNoise(z)
            eng.computeControl(cfg["x0"], 1)
            orc.colored_compute_control(cfg["x0"], 1, z, exps, decay, fmin)
        elif ctl == "robust":
            S = eng.STATE_DIM
            g = np.random.default_rng(5).uniform(-0.3, 0.3, (T, S, C)).astype(np.float32)
            if philox:
                eps = po.philox_normal(77, 0, K, T, C)[None]
            else:
                eps = host_noise(1, K, T, C, seed=K + T)
                eng.injectNoise(eps)
            # first cycle: no nominal state yet, no candidates (robust_mppi_controller.cu:508-633)
            eng.updateImportanceSamplingControl(cfg["x0"], 1)
            rob.update_importance_sampling(cfg["x0"], 1, None)
            eng.setFeedbackGains(g)
            rob.set_gains(g)
            if philox:
                eng.setSeed(77)
            eng.computeControl(cfg["x0"], 1)
            rob.compute_control(cfg["x0"], 1, eps)
        else:
            if philox:
                eng.setSeed(77)
                eps = po.philox_normal(77, 0, K, T, C)[None]
            else:
                eps = host_noise(1, K, T, C, seed=K + T)
                eng.injectNoise(eps)
            eng.computeControl(cfg["x0"], 1)
            (orc.tube_compute_control if ctl == "tube" else orc.vanilla_compute_control)(cfg["x0"], 1, eps)

        info = eng.getLaunchInfo()
        got = {k: info[k] for k in ("family", "block", "rows_in_hbm")}
        assert got == case["expect"], "%s: launched %s, the case expects %s" % (tag, got, case["expect"])
        assert not info["streamed_merge"], tag  # one iteration: nothing to merge from a previous launch

        costs = eng.getSampledCostSeq()
        assert np.isfinite(costs).all(), tag
        dc = int(ulp_diff(costs, orc.costs()).max())
        assert dc == 0, "%s: sampled costs differ from the oracle by up to %d ulp" % (tag, dc)
        du = float(np.abs(eng.getControlSeq() - orc.control()).max())
        assert du <= U_TOL, "%s: u* differs from the oracle by %g" % (tag, du)
        if ctl in ("tube", "robust"):
            dn = float(np.abs(eng.getNominalControlSeq() - orc.nominal_control()).max())
            assert dn <= U_TOL, "%s: nominal u* differs from the oracle by %g" % (tag, dn)
        if ctl != "robust":
            # independent of the oracle: the softmin of the engine's own rollouts, in float64
            u_opt, v = eng.getOptimalControlSeq(), eng.getSampledControls()
            for z in range(eng.num_systems):
                want = _softmin64(costs[z], v[z], cfg["lambda_"])
                err = float(np.abs(u_opt[z] - want).max())
                bound = SOFTMIN_RTOL * max(1.0, float(np.abs(want).max()))
                assert err <= bound, "%s: system %d u* is %g from the float64 softmin of its own samples" % (tag, z, err)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_kernel_matrix(gpu, case):
    if case["refuse"]:
        with pytest.raises(m.MPPIError) as e:
            _make(case, 65, 3)
        assert e.value.status == case["refuse"], "%s: refused with %d, documented %d" % (case["id"], e.value.status,
                                                                                          case["refuse"])
        return
    for K, T in (KT_COLORED if case["controller"] == "colored" else KT):
        _run(case, K, T, philox=False)
    _run(case, *PHILOX_KT, philox=True)


@pytest.mark.gpu
def test_launch_info_before_first_launch_and_streamed_merge(gpu):
    """MPPI_ERR_STATE before any launch; the one-system pipeline reports its streamed merge on the second iteration"""
    from common import cartpole_cfg
    cfg = cartpole_cfg(K=256, T=20, soft=True, num_iters=2)
    eng = make_engine(cfg, kernel_variant=m.MPPI_KERNEL_PIPELINE)
    with pytest.raises(m.MPPIError) as e:
        eng.getLaunchInfo()
    assert e.value.status == 7
    eng.computeControl(cfg["x0"], 1)
    info = eng.getLaunchInfo()
    assert info == dict(family="pipeline", block=(64, 1, 1), rows_in_hbm=False, streamed_merge=True), info
    eng.close()
