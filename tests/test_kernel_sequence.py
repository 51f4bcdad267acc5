"""Every registered kernel form held to the oracle over a short run of calls, and everything a call hands back.

tests/test_kernel_matrix.py checks one call with one iteration per (K, T).  Here every runnable case of the same enumeration
(build_cases / BUILDERS / _make, not a second list) runs two sequences of 3 computeControl calls with num_iters = 3:
  - Philox: the in-kernel noise, K = 1049 (16 full blocks of 64 and one partial), T = 12 so that T*C % 4 == 0 — the
    condition under which a one-system 64x1x1 pipeline handle streams the merge (engine_iteration.hip: streamMergeApplies);
  - injected: host noise per call, K = 200, T = 9 (T*C ragged).
Colored cases take the spectrum equivalents (po.philox_spectrum, host_spectrum).  Between two calls both sides slide by the
optimisation stride (1, 2, 1), the plant advances `stride` steps under the engine's control with the oracle's model_step, and
both sides get that same next state.  Robust MPPI follows the reference sequence: updateImportanceSamplingControl before every
call (it is where that controller slides), the gains and candidate set of test_kernel_matrix._run.

The noise generation each launch draws is worked out from the engine, and the oracle is handed exactly that stream: every
rollout launch advances h->generation by one (launchRollout), setSeed and injectNoise reset it to 0, a Robust candidate
evaluation draws one generation of its own — except on the first cycle, which evaluates nothing (rmNominalStateAndStride) —
and injected noise is read from slab generation % n_eps_iters.  A wrong counter shows as a cost mismatch.

Per call the test asserts
  which path ran   the launched family / block / rows-in-HBM; streamed_merge against the expectation the case builder derives
                   from streamMergeApplies(); and mppi_get_launch_counts: 3 rollout launches per call, and per call 1 merge
                   launch on the streamed path (the in-kernel merges of iterations 2 and 3 launch nothing, the last records are
                   merged by combineKernel or by the merging control phase, each counted once) or 3 otherwise (one combine, or
                   one reference-order reduction, per iteration);
  the oracle       last-iteration costs 0 ulp; control (and nominal control) within 1e-5; baselines exact; normalisers within
                   1e-6 relative; Tube nominal_state_used equal; Robust getRMPPIState against RobustOracle.state().  The
                   handle held to this runs in MPPI_REDUCTION_REFERENCE_ORDER, the oracle's order: in the fused order u*
                   differs from the oracle's by rounding, the next iteration samples around that mean, and from the 2nd
                   iteration on its costs differ by a few ulp (measured: 2 ulp on Cartpole, first call).  In every
                   case a default (fused) handle runs beside it through the same sequence, held to the oracle's control
                   (1e-5, or a measured drift listed in FUSED_DRIFT), to the path checks, to float64 and to the trajectories;
  float64          (numpy here, sharing no code with the engine or the oracle) u* of the last iteration against the softmin of
                   the engine's own dumped costs and samples, the statistics against the reference formulas, and the control
                   hand-back against the Savitzky-Golay filter over a control history the test keeps itself — see stats64 and
                   smooth64 for the bounds;
  trajectories     getTargetStateSeq / getTargetOutputSeq / getNominalStateSeq bit for bit (NaN == NaN) against the oracle's
                   re-rollout of the engine's OWN control sequence from the engine's own initial state;
  streamed merge   where the fused handle streams the merge, a twin created with MPPI_AMD_NO_STREAM_MERGE=1: u*,
                   statistics, costs and trajectories bit-identical to the streamed handle on every call.

Constraints: every registered model keeps the base Dynamics::enforceConstraints (a deadband, then a clamp to the control
ranges: dynamics.cu:97-116; no model overrides it, the configurations set no deadband), so constrain64 is a numpy clip for all
of them and none needs the oracle's model code.  ColoredMPPI clamps control channel 1 only (constrain_mode 1).
"""
import numpy as np
import pytest

import mppi_generic_amd as m
import pyoracle as po
from common import PHILOX_SEED, U_TOL, di_cfg, host_noise, host_spectrum, ulp_diff
from kernel_forms import (BUILDERS, FUSED_DRIFT, build_cases, expects_streamed_merge, make_handles, registrations,
                          robust_gains)
from restate64 import (SG_TAPS, SOFTMIN_RTOL, bits_equal, constrain64, ranges, save_history64, slide64, smooth64, softmin64,
                       stats64, stats_of)

N_CALLS = 3
N_ITERS = 3
STRIDES = (1, 2, 1)  # optimisation stride of call c; calls 1 and 2 are preceded by a slide / plant advance of that many steps
PHILOX_KT = (1049, 12)
INJECTED_KT = (200, 9)
NORM_RTOL_ORACLE = 1e-6


# ------------------------------------------------------------------ cases -----------------------------------------------
def _control_dim(model):
    return len(BUILDERS[model](1, 1, 1)["std_dev"])


def sequence_cases():
    regs = {(n, s): d for n, s, d in registrations()}
    dims = {}
    out = []
    for case in build_cases():
        if case["refuse"]:
            continue
        sampler = m.MPPI_SAMPLER_COLORED if case["controller"] == "colored" else m.MPPI_SAMPLER_GAUSSIAN
        d = regs[(case["model"], sampler)]
        C = dims.setdefault(case["model"], _control_dim(case["model"]))
        # stream: does the case's FUSED handle stream the merge in each sequence (the reference-order handle never does)
        out.append(dict(case, C=C, stream=dict(philox=expects_streamed_merge(case, d, *PHILOX_KT, C, True),
                                               injected=expects_streamed_merge(case, d, *INJECTED_KT, C, False))))
    return out


SEQ_CASES = sequence_cases()


# ------------------------------------------------------------------ CPU ------------------------------------------------
def test_every_streamed_merge_registration_has_a_streamed_case(lib):
    """a registration whose describe_model reports both the role pipeline and the streamed merge must have a case whose
    Philox sequence expects the streamed merge — else the STREAM_MERGE instantiation of its rolloutPipelineKernel is never run"""
    cases = sequence_cases()
    assert len(cases) == len([c for c in build_cases() if not c["refuse"]])
    for name, sampler, d in registrations():
        if not (d["pipeline"] and d["streamed_merge"]):
            continue
        prefix = name + ("[colored]" if sampler else "") + "-"
        mine = [c for c in cases if c["id"].startswith(prefix) and c["stream"]["philox"]]
        assert mine, "registration %s supports the streamed merge but no sequence case expects it" % prefix
    assert not any(c["stream"]["injected"] for c in cases)  # injected noise never streams


def test_streamed_merge_expectation_follows_each_condition(lib):
    d = dict(streamed_merge=True)
    base = dict(controller="vanilla", expect=dict(family="pipeline", block=(64, 1, 1), rows_in_hbm=False))
    assert expects_streamed_merge(base, d, 1049, 12, 1, True)
    assert not expects_streamed_merge(base, d, 1049, 9, 1, True)            # T*C % 4
    assert expects_streamed_merge(base, d, 1049, 9, 4, True)
    assert not expects_streamed_merge(base, d, 1049, 12, 1, False)          # injected noise
    assert not expects_streamed_merge(base, d, 1049, 12, 1, True, False)    # reference-order reduction
    assert not expects_streamed_merge(base, d, 64 * 257, 12, 1, True)       # more than 256 blocks
    assert not expects_streamed_merge(base, dict(streamed_merge=False), 1049, 12, 1, True)
    for ctl in ("tube", "robust"):
        assert not expects_streamed_merge(dict(base, controller=ctl), d, 1049, 12, 1, True)
    for e in (dict(family="pipeline", block=(64, 1, 1), rows_in_hbm=True), dict(family="pipeline", block=(32, 1, 1),
                                                                                 rows_in_hbm=False),
              dict(family="fused", block=(64, 1, 1), rows_in_hbm=False)):
        assert not expects_streamed_merge(dict(base, expect=e), d, 1049, 12, 1, True)


def _oracle_stats(costs, lambda_):
    """the oracle's statistics of one system from fp32 costs (the reference's own fp32 statement)"""
    base = po.baseline(costs)
    w = po.norm_exp(costs, np.float32(1.0 / lambda_), base)
    fe = po.free_energy(w, base, lambda_)
    return dict(baseline=base, normalizer=po.normalizer(w), free_energy_mean=fe[0], free_energy_variance=fe[1],
                free_energy_modified_variance=fe[2])


@pytest.mark.parametrize("K,spread,lambda_", [(1049, 30.0, 2.0), (200, 5.0, 0.25), (1, 3.0, 1.0), (64, 0.0, 1.0),
                                              (1049, 400.0, 0.5), (333, 1e4, 20.0)])
def test_stats64_against_the_oracle(K, spread, lambda_):
    """random costs, all costs equal (spread 0), a single rollout, and spreads far beyond 88 lambda (every weight but the
    best ones underflows in fp32)"""
    rng = np.random.default_rng(K)
    costs = (100.0 + spread * rng.random(K)).astype(np.float32)
    want, bound = stats64(costs, lambda_)
    got = _oracle_stats(costs, lambda_)
    for k in want:
        assert abs(got[k] - want[k]) <= bound[k], (k, got[k], want[k], bound[k])


def test_stats64_edges():
    c = np.full(50, 7.5, np.float32)
    v, b = stats64(c, 0.3)
    assert v["baseline"] == 7.5 and v["normalizer"] == 50
    assert abs(v["free_energy_mean"] - 7.5) <= 1e-12 and v["free_energy_variance"] == 0 and v["free_energy_modified_variance"] == 0
    # one dominant rollout: every other weight underflows (a spread of 1000 lambda), the statistics are the best rollout's
    c = np.concatenate([[3.0], np.full(99, 3.0 + 1000 * 0.3)]).astype(np.float32)
    v, b = stats64(c, 0.3)
    assert v["normalizer"] == 1.0
    assert abs(v["free_energy_mean"] - (-0.3 * np.log(1 / 100) + 3.0)) <= 1e-12
    g = _oracle_stats(c, 0.3)
    for k in v:
        assert abs(g[k] - v[k]) <= b[k], k


def test_softmin64_edges():
    rng = np.random.default_rng(1)
    v = rng.standard_normal((5, 4, 2))
    assert np.allclose(softmin64(np.full(5, 2.0), v, 1.0), v.mean(0), rtol=0, atol=1e-15)     # all costs equal
    c = np.array([10.0, 10.0 + 200, 10.0 + 300, 10.0 + 1e4, 10.0 + 89 * 0.5])
    assert np.array_equal(softmin64(c, v, 1.0), v[0])                                        # beyond 88 lambda: one rollout
    assert np.abs(softmin64(c, v, 0.5) - v[0]).max() < 1e-18 * np.abs(v).max() + 1e-15
    assert np.array_equal(softmin64(c[:1], v[:1], 1.0), v[0])                                # K = 1


@pytest.mark.parametrize("T,C", [(1, 1), (2, 2), (9, 2), (12, 3), (100, 1)])
def test_smooth64_against_the_oracle(T, C):
    rng = np.random.default_rng(T * 10 + C)
    for scale in (1.0, 1e-3, 50.0):
        u = (scale * rng.standard_normal((T, C))).astype(np.float32)
        h = (scale * rng.standard_normal((2, C))).astype(np.float32)
        want, bound = smooth64(u, h)
        got = po.smooth(u, h)
        assert (np.abs(got - want) <= bound).all(), np.abs(got - want).max()
        # the bound is tight enough to see one tap off by one place (the centre tap 17 -> 16 or 18: 1/35 of an input)
        for j, delta in ((2, 1.0), (2, -1.0), (0, 1.0)):
            taps = SG_TAPS.copy()
            taps[j] += delta / 35.0
            buf = np.concatenate([h.astype(np.float64), u, u[-1:], u[-1:]])
            bad = sum(taps[i] * buf[i:i + T] for i in range(5))
            assert not (np.abs(got - bad) <= bound).all(), (j, delta)


def test_smooth64_reference_known_answers():
    """controller_generic_tests.cu:214-238 (the values of test_oracle_kat.py)"""
    hist = np.zeros((2, 3), np.float32)
    s, b = smooth64(np.ones((1, 3), np.float32), hist)
    assert np.all(np.abs(s[0] - (17 + 12 - 3) / 35.0) <= 1e-15)
    s, b = smooth64(np.stack([np.ones(3), 2 * np.ones(3)]), hist)
    assert np.all(np.abs(s[0] - (17 + 24 - 6) / 35.0) <= 1e-15)
    assert np.all(np.abs(s[1] - (12 + 34 + 24 - 6) / 35.0) <= 1e-15)


@pytest.mark.parametrize("T,C", [(1, 1), (2, 2), (9, 2), (100, 2)])
def test_slide_and_history64_against_the_oracle(T, C):
    rng = np.random.default_rng(T)
    u = rng.standard_normal((T, C)).astype(np.float32)
    h = rng.standard_normal((2, C)).astype(np.float32)
    for steps in sorted({0, 1, 2, T - 1, T}):
        assert np.array_equal(slide64(u, steps), po.slide(u, steps)), steps
        zero, scale = rng.standard_normal(C).astype(np.float32), rng.uniform(0, 1, C).astype(np.float32)
        np.testing.assert_allclose(slide64(u, steps, zero, scale), po.slide(u, steps, zero, scale), rtol=1e-6, atol=1e-6)
        if steps <= T:
            assert np.array_equal(save_history64(steps, u, h), po.save_history(steps, u, h)), steps


def test_slide_and_history64_reference_known_answers():
    """controller_generic_tests.cu:240-283 and controller.cuh:602-615 (the values of test_oracle_kat.py)"""
    T = 100
    u = np.repeat(np.arange(T, dtype=np.float64)[:, None], 2, 1)
    u = slide64(u, 1)
    assert all(np.all(u[i] == (0 if i + 1 > T - 1 else i + 1)) for i in range(T))
    u = slide64(u, 10)
    assert all(np.all(u[i] == (0 if i + 10 > T - 2 else min(i + 11, T - 1))) for i in range(T))
    u = np.arange(20, dtype=np.float64).reshape(10, 2)
    h = np.array([[100, 101], [200, 201]], np.float64)
    assert np.array_equal(save_history64(1, u, h), [[200, 201], [0, 1]])
    assert np.array_equal(save_history64(3, u, h), [[2, 3], [4, 5]])
    assert np.array_equal(save_history64(0, u, h), h)


def test_constrain64():
    u = np.array([[-3.0, 0.5], [0.2, 9.0]])
    lo_hi = (np.array([-1.0, -2.0]), np.array([1.0, 2.0]))
    assert np.array_equal(constrain64(u, lo_hi), [[-1.0, 0.5], [0.2, 2.0]])
    assert np.array_equal(constrain64(u, lo_hi, channels=[1]), [[-3.0, 0.5], [0.2, 2.0]])


# ------------------------------------------------------------------ GPU ------------------------------------------------
def _fused_pair(case, K, T):
    """(streamed handle, two-launch twin) in the default fused reduction; MPPI_AMD_NO_STREAM_MERGE is read at mppi_create"""
    _, streamed, _, _ = make_handles(case, K, T, num_iters=N_ITERS)
    _, twin, _, _ = make_handles(case, K, T, num_iters=N_ITERS, env=dict(MPPI_AMD_NO_STREAM_MERGE="1"))
    return streamed, twin


def _observe(eng, ctl, has_outputs):
    """everything a call hands back, for the streamed / two-launch comparison"""
    st = eng.getStats()
    out = dict(u=eng.getControlSeq(), u_opt=eng.getOptimalControlSeq(), costs=eng.getSampledCostSeq(),
               x=eng.getTargetStateSeq(), stats=np.array(list(stats_of(st, "real_sys").values()), np.float32))
    if has_outputs:
        out["y"] = eng.getTargetOutputSeq()
    return out


class _Handle:
    """one engine handle of a sequence and the control history the test keeps for it"""

    def __init__(self, eng, role, streamed, C):
        self.e, self.role, self.streamed = eng, role, streamed
        self.counts0 = None
        self.hist = np.zeros((2, C))   # what the smoothing reads (Robust: the real system's history)
        self.nhist = np.zeros((2, C))  # Robust: the nominal system's
        self.u = self.un = None        # the control (and nominal control) the last call handed back
        self.drift = 0.0               # fused handles: the largest control difference from the oracle so far


def _check_handle(h, case, cfg, orc, x, call, tag, exact):
    """every per-call assertion on one handle; exact: the handle reduces in the oracle's order (costs 0 ulp, baselines
    exact, normalisers 1e-6) — the fused handles start their 2nd and 3rd iteration from a u* that differs from the oracle's
    by rounding, so only their control is held to the oracle (1e-5) and everything else to float64 and to each other"""
    e, ctl = h.e, case["controller"]
    tag = "%s [%s]" % (tag, h.role)
    C, O = e.CONTROL_DIM, e.OUTPUT_DIM
    lam = cfg["lambda_"]
    # -------- which path ran
    info = e.getLaunchInfo()
    got = {k: info[k] for k in ("family", "block", "rows_in_hbm")}
    assert got == case["expect"], "%s: launched %s, the case expects %s" % (tag, got, case["expect"])
    assert info["streamed_merge"] == h.streamed, "%s: streamed_merge %s, expected %s" % (tag, info["streamed_merge"],
                                                                                         h.streamed)
    r, g = e.launchCounts()
    n = call + 1
    want_counts = (N_ITERS * n, (1 if h.streamed else N_ITERS) * n)
    got_counts = (r - h.counts0[0], g - h.counts0[1])
    assert got_counts == want_counts, "%s: (rollout, merge) launches %s, the %s path implies %s" % (
        tag, got_counts, "streamed" if h.streamed else "two-launch", want_counts)

    # -------- against the oracle
    costs = e.getSampledCostSeq()
    assert np.isfinite(costs).all(), tag
    if exact:
        dc = int(ulp_diff(costs, orc.costs()).max())
        assert dc == 0, "%s: sampled costs differ from the oracle by up to %d ulp" % (tag, dc)
    u = e.getControlSeq()
    du = float(np.abs(u - orc.control()).max())
    un = None
    dn = 0.0
    if ctl in ("tube", "robust"):
        un = e.getNominalControlSeq()
        dn = float(np.abs(un - orc.nominal_control()).max())
    if exact:
        assert du <= U_TOL, "%s: control differs from the oracle by %g" % (tag, du)
        assert dn <= U_TOL, "%s: nominal control differs from the oracle by %g" % (tag, dn)
    else:  # asserted once the sequence is over (_run_sequence), so that the message reports the drift of all 3 calls
        h.drift = max(h.drift, du, dn)
    st = e.getStats()
    ost = orc.stats()
    # system z of the handle -> the stats field: Robust's system 0 is the nominal one (robust_mppi_controller.cu:637)
    sysnames = (["nominal_sys", "real_sys"] if ctl == "robust" else ["real_sys", "nominal_sys"])[:e.num_systems]
    if exact:
        for z, name in enumerate(sysnames):
            s = stats_of(st, name)
            assert s["baseline"] == ost["baseline"][z], "%s: %s baseline %r, oracle %r" % (tag, name, s["baseline"],
                                                                                          ost["baseline"][z])
            rn = abs(s["normalizer"] - ost["normalizer"][z]) / abs(ost["normalizer"][z])
            assert rn <= NORM_RTOL_ORACLE, "%s: %s normaliser %g relative from the oracle" % (tag, name, rn)
        if ctl == "tube":
            assert st.nominal_state_used == ost["nominal_state_used"], "%s: nominal_state_used %d, oracle %d" % (
                tag, st.nominal_state_used, ost["nominal_state_used"])

    # -------- against float64, from the handle's own costs and samples
    u_opt, v = e.getOptimalControlSeq(), e.getSampledControls()
    for z, name in enumerate(sysnames):
        if ctl == "tube" and z == 1 and st.nominal_state_used == 0:
            # tubeSelectKernel: the actual system won the last pass, the nominal mean IS the actual one
            assert bits_equal(u_opt[1], u_opt[0], nan_equal=True), "%s: nominal u* after a take-over" % tag
        else:
            # Robust: row 0 of the dumped costs is the combined S_nom the nominal update weighs (rmppi_kernels.hpp)
            want = softmin64(costs[z], v[z], lam)
            err = float(np.abs(u_opt[z] - want).max())
            bound = SOFTMIN_RTOL * max(1.0, float(np.abs(want).max()))
            assert err <= bound, "%s: system %d u* is %g from the float64 softmin of its own samples" % (tag, z, err)
        want, bound = stats64(costs[z], lam)
        got = stats_of(st, name)
        for k in want:
            assert abs(got[k] - want[k]) <= bound[k], "%s: %s %s = %r, float64 %r (bound %g)" % (
                tag, name, k, got[k], want[k], bound[k])

    # smoothing (and constraints) of what the call hands back, from u* and the history kept here
    lo_hi = ranges(cfg, C)
    if ctl in ("vanilla", "colored"):
        sm, b = smooth64(u_opt[0], h.hist)
        want = sm if (ctl == "colored" and C == 1) else constrain64(sm, lo_hi, [1] if ctl == "colored" else None)
        checks = [("control", u, want, b)]
    elif ctl == "tube":
        # the actual control is handed back raw; the nominal one smoothed (tube_mppi_controller.cu:281), no clamp
        sm, b = smooth64(u_opt[1] if st.nominal_state_used else u_opt[0], h.hist)
        checks = [("control", u, u_opt[0].astype(np.float64), np.zeros_like(b)), ("nominal control", un, sm, b)]
    else:
        sm_n, bn = smooth64(u_opt[0], h.nhist)
        sm_r, br = smooth64(u_opt[1], h.hist)
        checks = [("control", u, sm_r, br), ("nominal control", un, sm_n, bn)]
    for what, got, want, b in checks:
        err = np.abs(np.asarray(got, np.float64) - want)
        assert (err <= b).all(), "%s: %s is %g from the float64 Savitzky-Golay filter of u* (bound %g)" % (
            tag, what, float(err.max()), float(b.flat[np.argmax(err - b)]))

    # -------- trajectories, re-rolled by the oracle from the handle's own control
    x_state = e.getTargetStateSeq()
    if ctl == "robust":
        # getTargetStateSeq is the nominal trajectory there, from the nominal state the candidates chose
        x0_n = e.getRMPPIState()[0]
        assert bits_equal(x_state, orc.state_trajectory(x0_n, un), nan_equal=True), "%s: nominal state trajectory" % tag
        assert bits_equal(e.getNominalStateSeq(), x_state, nan_equal=True), tag
        traj_x0, traj_u = x0_n, un
    else:
        assert bits_equal(x_state, orc.state_trajectory(x, u), nan_equal=True), "%s: state trajectory of the handed-back control" % tag
        traj_x0, traj_u = x, u
    if O > 0:
        _, y = orc.output_trajectory(traj_x0, traj_u)
        assert bits_equal(e.getTargetOutputSeq(), y, nan_equal=True), "%s: output trajectory" % tag
    if ctl == "tube":
        xn = e.getNominalStateSeq()
        if exact:
            assert bits_equal(xn[0], orc.nominal_state_traj()[0], nan_equal=True), "%s: nominal initial state" % tag
        assert bits_equal(xn, orc.state_trajectory(xn[0], un), nan_equal=True), "%s: nominal state trajectory" % tag
    h.u, h.un = u, un


def _run_sequence(case, mode):
    """3 calls of one case on two handles, or three where the merge streams.
      - reference order: MPPI_REDUCTION_REFERENCE_ORDER, the oracle's own order, held to it bit for bit (costs 0 ulp).  With
        the fused reduction u* differs from the oracle's by rounding, the 2nd iteration samples around that mean, and its
        costs can no longer be 0 ulp (measured: 2 ulp on Cartpole in the first call);
      - fused: the default configuration a caller runs (fused merge, streamed where streamMergeApplies() holds, the
        BAR-inbox hand-over where the device has one), held to the oracle's control (1e-5) and to every path, float64 and
        trajectory check;
      - two-launch (streamed cases only): the fused handle without the streamed merge, bit-identical to the streamed one."""
    philox = mode == "philox"
    K, T = PHILOX_KT if philox else INJECTED_KT
    ctl = case["controller"]
    tag0 = "%s %s K=%d T=%d" % (case["id"], mode, K, T)
    cfg, eng, orc, rob = make_handles(case, K, T, num_iters=N_ITERS)
    C, S, O = eng.CONTROL_DIM, eng.STATE_DIM, eng.OUTPUT_DIM
    handles = [_Handle(eng, "reference-order", False, C)]
    eng.setReductionMode(m.MPPI_REDUCTION_REFERENCE_ORDER)
    try:
        if case["stream"][mode]:
            streamed, twin = _fused_pair(case, K, T)
            handles += [_Handle(streamed, "fused, streamed", True, C), _Handle(twin, "fused, two-launch", False, C)]
        else:
            handles.append(_Handle(make_handles(case, K, T, num_iters=N_ITERS)[1], "fused", False, C))
        engines = [h.e for h in handles]
        assert C == case["C"], tag0
        if ctl == "colored":
            exps, decay, fmin = cfg["colored"]
        if ctl == "robust":
            gains = robust_gains(T, S, C)
        for h in handles:
            h.counts0 = h.e.launchCounts()
        if philox:
            for e in engines:
                e.setSeed(PHILOX_SEED)
        gen = 0  # the engine's h->generation, as worked out from launchRollout / rmNominalStateAndStride
        x = cfg["x0"].copy()
        for call in range(N_CALLS):
            stride = STRIDES[call]
            tag = "%s call %d" % (tag0, call)
            if call > 0:
                # the plant: `stride` steps under the control the exact handle handed back; every side starts from that state
                for s in range(stride):
                    x, _ = orc.model_step(x, handles[0].u[s])
                if ctl != "robust":
                    for h in handles:
                        h.e.slideControlSequence(stride)
                        h.hist = save_history64(stride, h.un if ctl == "tube" else h.u, h.hist)
                    (orc.tube_slide if ctl == "tube" else orc.vanilla_slide)(stride)
            # the noise of this call, in the order the engine's launches draw it
            slabs = z = None
            if not philox:
                gen = 0  # injectNoise resets the generation
                if ctl == "colored":
                    z = host_spectrum(N_ITERS, K, T, C, seed=1000 * call + K + T)
                else:
                    slabs = host_noise(N_ITERS, K, T, C, seed=1000 * call + K + T)
                for e in engines:
                    e.injectNoise(z if ctl == "colored" else slabs)
            elif ctl == "colored":
                z = np.stack([po.philox_spectrum(PHILOX_SEED, gen + i, K, T, C) for i in range(N_ITERS)])

            def draw(g):
                return po.philox_normal(PHILOX_SEED, g, K, T, C) if philox else slabs[g % N_ITERS]

            if ctl == "robust":
                # updateImportanceSamplingControl: candidate evaluation (one generation; none on the first cycle) and slide
                eps_is = None
                if call > 0:
                    eps_is = draw(gen)
                    gen += 1
                for e in engines:
                    e.updateImportanceSamplingControl(x, stride)
                rob.update_importance_sampling(x, stride, eps_is)
                if call == 0:
                    for e in engines:
                        e.setFeedbackGains(gains)
                    rob.set_gains(gains)
                ns_e, best_e, nstride_e, fe_e = eng.getRMPPIState()
                ns_o, best_o, nstride_o, fe_o = rob.state()
                assert (best_e, nstride_e) == (best_o, nstride_o), "%s: best candidate / stride %s, oracle %s" % (
                    tag, (best_e, nstride_e), (best_o, nstride_o))
                assert bits_equal(ns_e, ns_o, nan_equal=True), "%s: nominal state %s, oracle %s" % (tag, ns_e, ns_o)
                assert bits_equal(fe_e, fe_o, nan_equal=True), "%s: candidate free energies %s, oracle %s" % (tag, fe_e, fe_o)
                if call > 0:
                    for h in handles:  # (each handle's own candidate choice decides its nominal slide)
                        h.nhist = save_history64(h.e.getRMPPIState()[2], h.un, h.nhist)
                        h.hist = save_history64(stride, h.u, h.hist)
            if ctl != "colored":
                eps = np.stack([draw(gen + i) for i in range(N_ITERS)])
            gen += N_ITERS

            for e in engines:
                e.computeControl(x, stride)
            if ctl == "colored":
                orc.colored_compute_control(x, stride, z, exps, decay, fmin)
            elif ctl == "robust":
                rob.compute_control(x, stride, eps)
            elif ctl == "tube":
                orc.tube_compute_control(x, stride, eps)
            else:
                orc.vanilla_compute_control(x, stride, eps)

            for i, h in enumerate(handles):
                _check_handle(h, case, cfg, orc, x, call, tag, exact=i == 0)
            # the streamed merge is the two-launch iteration: everything handed back, bit for bit
            if len(handles) == 3:
                a, b = _observe(handles[1].e, ctl, O > 0), _observe(handles[2].e, ctl, O > 0)
                for k in a:
                    assert bits_equal(a[k], b[k], nan_equal=True), "%s: %s of the streamed handle differs from the two-launch twin" % (tag, k)
        bound = FUSED_DRIFT.get((case["id"], mode), U_TOL)
        for h in handles[1:]:
            assert h.drift <= bound, "%s [%s]: control differs from the oracle by up to %g over the %d calls (bound %g)" % (
                tag0, h.role, h.drift, N_CALLS, bound)
    finally:
        for h in handles:
            h.e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", SEQ_CASES, ids=[c["id"] for c in SEQ_CASES])
def test_kernel_sequence(gpu, case):
    _run_sequence(case, "philox")
    _run_sequence(case, "injected")


@pytest.mark.gpu
@pytest.mark.parametrize("controller", [m.VanillaMPPIController, m.TubeMPPIController, m.RobustMPPIController])
def test_compute_control_refuses_a_state_of_the_wrong_size(gpu, controller):
    """mppi_compute_control reads STATE_DIM floats for every controller; any other size is MPPI_ERR_INVALID_ARG, never a
    read of the staging array's stale tail (short state) or a silently dropped one (long state)"""
    cfg = di_cfg(K=256, T=8, tube=controller is not m.VanillaMPPIController)
    eng = controller(cfg["model"], cfg["K"], cfg["T"], cfg["dt"], cfg["lambda_"])
    try:
        S = eng.STATE_DIM
        for n in (0, S - 1, S + 1, 2 * S + 1, 2 * S):
            with pytest.raises(m.MPPIError) as e:
                eng.computeControl(np.ones(n, np.float32), 1)
            assert e.value.status == m.MPPI_ERR_INVALID_ARG, (n, e.value.status)
        if controller is m.RobustMPPIController:  # updateImportanceSamplingControl reads a state of STATE_DIM floats too
            for n in (0, S - 1, S + 1, 2 * S + 1, 2 * S):
                with pytest.raises(m.MPPIError) as e:
                    eng.updateImportanceSamplingControl(np.ones(n, np.float32), 1)
                assert e.value.status == m.MPPI_ERR_INVALID_ARG, (n, e.value.status)
            eng.updateImportanceSamplingControl(np.ones(S, np.float32), 1)
        else:  # (Robust needs its gains first)
            eng.computeControl(np.ones(S, np.float32), 1)
            eng.computeControl(np.ones((1, S), np.float32), 1)
    finally:
        eng.close()
