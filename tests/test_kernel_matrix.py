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
import numpy as np
import pytest

import mppi_generic_amd as m
import pyoracle as po
from common import PHILOX_SEED, U_TOL, cartpole_cfg, host_noise, host_spectrum, make_engine
from kernel_forms import BUILDERS, KT, build_cases, check_against_oracle, check_form, compute_once, make_handles, registrations
from restate64 import SOFTMIN_RTOL, softmin64

KT_COLORED = KT + [(65, 16), (200, 17)]
PHILOX_KT = (65, 5)


# ------------------------------------------------------------------ CPU ------------------------------------------------
def test_every_registration_has_a_builder_and_cases(lib):
    """fails when a registered model has no configuration builder here (a new model cannot skip parity), when a
    registration yields no case, or when mppi_describe_model disagrees with the registration's own listing"""
    regs = registrations()
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
    assert lib.mppi_describe_model(b"cartpole", 7, None, 0, None, None) == m.MPPI_ERR_INVALID_ARG
    n = C.c_int()
    assert lib.mppi_describe_model(b"cartpole", 0, None, 0, C.byref(n), None) == m.MPPI_OK and n.value == len(d["shapes"])


# ------------------------------------------------------------------ GPU ------------------------------------------------
CASES = build_cases()


def _run(case, K, T, philox):
    """one (K, T) of a case; returns nothing, asserts with the case's name in every message"""
    tag = "%s K=%d T=%d%s" % (case["id"], K, T, " philox" if philox else "")
    if case["controller"] == "robust" and K < 3:
        # RobustMPPIController needs at least 3 candidates x 1 sample (robust_mppi_controller.cu: candidates odd, >= 3)
        with pytest.raises(m.MPPIError) as e:
            make_handles(case, K, T)
        assert e.value.status == m.MPPI_ERR_INVALID_ARG, "%s: refused with %d" % (tag, e.value.status)
        return
    cfg, eng, orc, rob = make_handles(case, K, T)
    try:
        C, ctl = eng.CONTROL_DIM, case["controller"]
        if ctl == "colored":
            noise = po.philox_spectrum(PHILOX_SEED, 0, K, T, C)[None] if philox else host_spectrum(1, K, T, C, seed=K + T)
        else:
            noise = po.philox_normal(PHILOX_SEED, 0, K, T, C)[None] if philox else host_noise(1, K, T, C, seed=K + T)
        compute_once(case, [eng], orc, rob, cfg, 1, noise, philox, PHILOX_SEED, seed_before_first_cycle=False)

        check_form(case, eng, tag)  # (one iteration: nothing to merge from a previous launch, streamed_merge is False)
        du = check_against_oracle(case, eng, orc, tag)
        assert du <= U_TOL, "%s: u* (or the nominal u*) differs from the oracle by %g" % (tag, du)
        if ctl != "robust":
            # independent of the oracle: the softmin of the engine's own rollouts, in float64
            costs, u_opt, v = eng.getSampledCostSeq(), eng.getOptimalControlSeq(), eng.getSampledControls()
            for z in range(eng.num_systems):
                want = softmin64(costs[z], v[z], cfg["lambda_"])
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
            make_handles(case, 65, 3)
        assert e.value.status == case["refuse"], "%s: refused with %d, documented %d" % (case["id"], e.value.status,
                                                                                          case["refuse"])
        return
    for K, T in (KT_COLORED if case["controller"] == "colored" else KT):
        _run(case, K, T, philox=False)
    _run(case, *PHILOX_KT, philox=True)


@pytest.mark.gpu
def test_launch_info_before_first_launch_and_streamed_merge(gpu):
    """MPPI_ERR_STATE before any launch; the one-system pipeline reports its streamed merge on the second iteration"""
    cfg = cartpole_cfg(K=256, T=20, soft=True, num_iters=2)
    eng = make_engine(cfg, kernel_variant=m.MPPI_KERNEL_PIPELINE)
    with pytest.raises(m.MPPIError) as e:
        eng.getLaunchInfo()
    assert e.value.status == m.MPPI_ERR_STATE
    eng.computeControl(cfg["x0"], 1)
    info = eng.getLaunchInfo()
    assert info == dict(family="pipeline", block=(64, 1, 1), rows_in_hbm=False, streamed_merge=True), info
    eng.close()
