"""The softmin reductions held to float64 at infinite, tied and far-apart costs.

The kernel-form files assert finite costs before anything else (kernel_forms.check_against_oracle, test_kernel_sequence.
_check_handle) and the written-record merge test keeps its records out of the subnormal band, so the rules the engine states
for these inputs ran nowhere: weight 0 for a rollout whose S - rho_b is NaN (rollout_kernel.hpp), scale 0 for an all-+inf
record (merge_wave.hpp: mergeScale), IEEE `/` outside [2^-60, 2^60) (mergeQuotients), det::exp == 0 at -104 and below, and
`inf < gamma` being false in the Tsallis weights.  Here they run, on the two double-integrator models only (plain arithmetic:
a non-finite value cannot become an address); tests/softmin_cases.py builds the scenarios.

CPU part   every scenario's design asserted from the oracle's costs, for every (model, controller) and shape the GPU part
           uses: a scenario whose inputs miss their design fails here, not on the GPU.  The +inf-aware float64 twins
           (softmin64_inf, stats64_inf) equal restate64's on finite inputs and hold the oracle's own baseline / norm_exp /
           normalizer / free_energy on every scenario's costs; their bounds are finite whenever the value is.
GPU part   every runnable case of build_cases() of the two models x every scenario: a reference-order handle, a fused handle,
           the MPPI_AMD_NO_STREAM_MERGE twin where the merge streams, the MPPI_AMD_NO_MERGE_CONTROL twin on Vanilla cases, one
           Tsallis run on the colored cases; then the gathered merge on written edge records and the unfused operators.
"""
import numpy as np
import pytest

import mppi_generic_amd as m
import pyoracle as po
from common import PHILOX_SEED, U_TOL, make_engine
from kernel_forms import build_cases, check_form, expects_streamed_merge, registrations, robust_gains
from restate64 import SOFTMIN_RTOL, bits_equal, softmin64, stats64, stats_of
from softmin_cases import (ALL_INF, EDGE_MERGE_SETS, FAR_BLOCK, INJECTED, INJECTED_KT, MODELS, NON_FINITE, PHILOX, PHILOX_ITERS,
                           PHILOX_KT, RECORD_EDGE_KT, SUBNORMAL_FLOOR, ZERO_WEIGHT_RERUN, edge_merge_records, oracle_costs,
                           scale_arg32, scale_second_channel, scenario, scenario_handles, softmin64_inf, stats64_inf)
from test_sharded_matrix import (MERGE_LAMBDA, MERGE_PROBLEMS, MERGE_WORLDS, UNIT, _merge_cfg, _merge_once, _merge_reference,
                                 _merge_x)

NORM_RTOL_ORACLE = 1e-6        # the constant tests/test_kernel_sequence.py uses
TSALLIS = (400.0, 1.7)         # gamma, r_exp of tests/test_reference_order_reduction.py
TSALLIS_SCENARIOS = ("mixed_inf", "one_finite", "all_inf")
STAT_KEYS = ("baseline", "normalizer", "free_energy_mean", "free_energy_variance", "free_energy_modified_variance")


def edge_cases():
    return [c for c in build_cases() if c["model"] in MODELS and not c["refuse"]]


CASES = edge_cases()
REGS = {(n, s): d for n, s, d in registrations()}
CONTROLLER_KINDS = sorted({(c["model"], c["controller"]) for c in CASES})


def _kind_case(model, ctl):
    return dict(model=model, controller=ctl)


def _record_edge(case):
    """the fused 16x1x1 / 16x1x2 cases: K = 4096 and 4112 give 256 and 257 block records"""
    e = case.get("expect")
    return bool(e) and e["family"] == "fused" and e["block"][:2] == (16, 1) and not e["rows_in_hbm"]


def shapes_of(name, ctl, record_edge):
    """the (K, T) a scenario runs at; all_tied needs a K that is no multiple of 64"""
    if name in PHILOX:
        return [PHILOX_KT]
    out = [INJECTED_KT] + (RECORD_EDGE_KT if record_edge else [])
    return [kt for kt in out if not (name == "all_tied" and kt[0] % 64 == 0)]


# ------------------------------------------------------------------ CPU: the scenarios' design --------------------------
def _blocks(mask, n):
    """per block of n rollouts: (all, any) of a boolean mask [K]"""
    K = mask.size
    return [(bool(mask[i:i + n].all()), bool(mask[i:i + n].any())) for i in range(0, K, n)]


def check_design(name, sc, costs, lam, tag):
    """the "what must hold for the inputs" column, per system, from the oracle's costs [D][K]"""
    K = costs.shape[1]
    assert not np.isnan(costs).any(), "%s: a NaN cost" % tag
    for z, c in enumerate(costs):
        inf = np.isposinf(c)
        if name in ("mixed_inf", "overflow"):
            assert np.array_equal(np.flatnonzero(inf), sc["rows"]), "%s system %d: +inf at %s" % (tag, z, np.flatnonzero(inf))
            for n in (64, 32, 16):
                assert any(a for a, _ in _blocks(inf, n)), "%s: no all-+inf block of %d" % (tag, n)
            assert any(y and not a for a, y in _blocks(inf, 64)), "%s: no mixed block" % tag
            assert np.isfinite(c.min()), tag
            if name == "overflow":
                assert np.isfinite(sc["overlay"]["cost"].crash_cost), tag  # +inf is reached by accumulation alone
        elif name == "one_finite":
            assert int(np.isfinite(c).sum()) == 1, "%s system %d: %d finite costs" % (tag, z, int(np.isfinite(c).sum()))
        elif name in ALL_INF:
            assert inf.all(), "%s system %d: %d costs are not +inf" % (tag, z, int((~inf).sum()))
        elif name == "tied_min":
            assert np.isfinite(c).all(), tag
            tied = np.flatnonzero(c.view(np.uint32) == c[np.argmin(c)].view(np.uint32))
            assert tied.size >= 4 and len(set(tied // 64)) >= 3, "%s system %d: the minimum is attained at %s" % (tag, z, tied)
        elif name == "all_tied":
            assert K % 64 != 0 and np.isfinite(c).all(), tag
            assert (c[1:].view(np.uint32) == c[1].view(np.uint32)).all(), "%s system %d: the noise-taking rollouts are not tied" % (tag, z)
        elif name in ("far_zero", "far_subnormal"):
            assert np.isfinite(c).all(), tag
            x = scale_arg32(c[FAR_BLOCK].min(), c.min(), lam)
            if name == "far_zero":
                assert x > 104.0, "%s system %d: the all-crash block is %g lambda above the minimum" % (tag, z, x)
            else:
                assert 88.0 < x < 103.0, "%s system %d: the all-crash block is %g lambda above the minimum" % (tag, z, x)
        elif name == "philox_mixed":
            share = float(inf.mean())
            assert 0.25 <= share <= 0.75 and np.isfinite(c.min()), "%s system %d: +inf share %g" % (tag, z, share)


def _lambda_of(sc):
    return sc["overlay"].get("lambda_", 2.0)  # di_cfg / robust_cfg default


def _scenario_costs(kind, name, K, T):
    """[(tag, costs [D][K])] of a scenario: one entry, or one per iteration run for the Philox scenarios"""
    sc = scenario(name, kind, K, T)
    if not sc["philox"]:
        return sc, [("", oracle_costs(kind, K, T, sc["overlay"], sc["noise"]))]
    out = [(" iteration %d" % n, oracle_costs(kind, K, T, sc["overlay"], sc["noise"][:n], num_iters=n))
           for n in range(1, (1 if name in ALL_INF else PHILOX_ITERS) + 1)]
    return sc, out


@pytest.mark.parametrize("name", INJECTED + PHILOX)
@pytest.mark.parametrize("model,ctl", CONTROLLER_KINDS, ids=["%s-%s" % k for k in CONTROLLER_KINDS])
def test_scenario_design(lib, model, ctl, name):
    kind = _kind_case(model, ctl)
    for K, T in shapes_of(name, ctl, record_edge=ctl in ("vanilla", "tube")):
        sc, runs = _scenario_costs(kind, name, K, T)
        for it, costs in runs:
            tag = "%s-%s %s K=%d T=%d%s" % (model, ctl, name, K, T, it)
            assert costs.shape == (2 if ctl in ("tube", "robust") else 1, K), tag
            check_design(name, sc, costs, _lambda_of(sc), tag)
            # the extended float64 statistics: finite bounds whenever the value is finite (an infinite bound hides any failure)
            for c in costs:
                vals, bounds = stats64_inf(c, _lambda_of(sc))
                for k in STAT_KEYS:
                    assert np.isfinite(bounds[k]), "%s: %s has the bound %r" % (tag, k, bounds[k])
                    if name not in ALL_INF:
                        assert np.isfinite(vals[k]), "%s: %s = %r" % (tag, k, vals[k])
                assert (vals["baseline"] == np.inf) == (name in ALL_INF), tag


def test_every_form_of_the_two_models_is_a_case(lib):
    """the cases are build_cases() filtered to the two models, every reduction form among them"""
    assert [c["id"] for c in edge_cases()] == [c["id"] for c in build_cases() if c["model"] in MODELS and not c["refuse"]]
    fams = {(c["expect"]["family"], c["expect"]["block"], c["expect"]["rows_in_hbm"]) for c in CASES}
    for want in (("fused", (64, 1, 1), False), ("fused", (16, 1, 1), False), ("fused", (16, 1, 2), False), ("fused", (64, 1, 2), False),
                 ("pipeline", (64, 1, 1), False), ("pipeline_fold", (32, 1, 2), False), ("fused", (64, 1, 1), True),
                 ("rmppi", (64, 1, 2), False), ("rmppi_pipeline", (64, 1, 2), True)):
        assert want in fams, want
    assert {c["controller"] for c in CASES} == {"vanilla", "tube", "robust", "colored"}
    assert sum(_record_edge(c) for c in CASES) == 4   # 16x1x1 and 16x1x2 of each model
    streamed = [c["id"] for c in CASES if _streams(c, "philox_mixed")]
    assert len(streamed) == 2, streamed              # the one-system 64x1x1 pipeline of each model


# ------------------------------------------------------------------ CPU: the float64 twins ------------------------------
@pytest.mark.parametrize("K,spread,lambda_", [(1049, 30.0, 2.0), (200, 5.0, 0.25), (1, 3.0, 1.0), (64, 0.0, 1.0),
                                              (1049, 400.0, 0.5), (333, 1e4, 20.0)])
def test_twins_equal_restate64_on_finite_costs(K, spread, lambda_):
    rng = np.random.default_rng(K)
    costs = (100.0 + spread * rng.random(K)).astype(np.float32)
    v = rng.standard_normal((K, 3, 2))
    assert np.array_equal(softmin64_inf(costs, v, lambda_), softmin64(costs, v, lambda_))
    (want, wb), (got, gb) = stats64(costs, lambda_), stats64_inf(costs, lambda_)
    for k in STAT_KEYS:
        assert got[k] == want[k] and gb[k] == wb[k], (k, got[k], want[k], gb[k], wb[k])


def test_twins_rules_for_infinite_costs():
    rng = np.random.default_rng(3)
    v = rng.standard_normal((6, 4, 2))
    c = np.array([5.0, np.inf, 6.0, np.inf, np.inf, 5.5])
    fin = np.isfinite(c)
    # weight 0, whatever the samples are ...
    assert np.array_equal(softmin64_inf(c, v, 0.7), softmin64(c[fin], v[fin], 0.7))
    v2 = v.copy()
    v2[~fin] = 1e30
    assert np.array_equal(softmin64_inf(c, v2, 0.7), softmin64_inf(c, v, 0.7))
    # ... and still counted in K: the normaliser is the finite rollouts', the free energy is of the mean over all 6
    vals, bounds = stats64_inf(c, 0.7)
    fv, _ = stats64(c[fin], 0.7)
    assert vals["baseline"] == 5.0 and vals["normalizer"] == fv["normalizer"]
    assert abs(vals["free_energy_mean"] - (-0.7 * np.log(fv["normalizer"] / 6) + 5.0)) <= 1e-12
    assert all(np.isfinite(b) for b in bounds.values())
    # one finite cost: normaliser exactly 1, u* that rollout's sample
    c1 = np.full(6, np.inf)
    c1[4] = 2.5
    assert np.array_equal(softmin64_inf(c1, v, 0.7), v[4]) and stats64_inf(c1, 0.7)[0]["normalizer"] == 1.0
    # nothing has weight: baseline +inf, NaN
    vals, bounds = stats64_inf(np.full(6, np.inf), 0.7)
    assert vals["baseline"] == np.inf and all(np.isnan(vals[k]) for k in STAT_KEYS[1:])
    assert np.isnan(softmin64_inf(np.full(6, np.inf), v, 0.7)).all()


def _oracle_stats(costs, lambda_):
    """the oracle's statistics of one system from fp32 costs (the reference's own fp32 statement)"""
    base = po.baseline(costs)
    w = po.norm_exp(costs, np.float32(1.0 / lambda_), base)
    fe = po.free_energy(w, base, lambda_)
    return w, dict(baseline=base, normalizer=po.normalizer(w), free_energy_mean=fe[0], free_energy_variance=fe[1],
                   free_energy_modified_variance=fe[2])


@pytest.mark.parametrize("name", INJECTED + PHILOX)
@pytest.mark.parametrize("model,ctl", CONTROLLER_KINDS, ids=["%s-%s" % k for k in CONTROLLER_KINDS])
def test_twins_against_the_oracle_on_scenario_costs(lib, model, ctl, name):
    """in the style of test_stats64_against_the_oracle, on the costs every scenario really has"""
    kind = _kind_case(model, ctl)
    for K, T in shapes_of(name, ctl, record_edge=ctl in ("vanilla", "tube")):
        sc, runs = _scenario_costs(kind, name, K, T)
        lam = _lambda_of(sc)
        for it, costs in runs:
            for z, c in enumerate(costs):
                tag = "%s-%s %s K=%d T=%d%s system %d" % (model, ctl, name, K, T, it, z)
                want, bound = stats64_inf(c, lam)
                w, got = _oracle_stats(c, lam)
                assert got["baseline"] == want["baseline"], tag
                if name in ALL_INF:
                    # the reference's norm_exp is exp(-(inf - inf) / lambda): NaN weights, nothing else to hold
                    assert np.isnan(w).all() and np.isnan(got["normalizer"]), tag
                    continue
                assert (w[np.isposinf(c)] == 0).all(), "%s: a +inf cost with a weight" % tag
                for k in STAT_KEYS:
                    assert abs(got[k] - want[k]) <= bound[k], "%s: %s = %r, float64 %r (bound %g)" % (tag, k, got[k], want[k], bound[k])


# ------------------------------------------------------------------ GPU: every reduction form ---------------------------
def _streams(case, name):
    if name not in PHILOX:
        return False
    sampler = m.MPPI_SAMPLER_COLORED if case["controller"] == "colored" else m.MPPI_SAMPLER_GAUSSIAN
    return expects_streamed_merge(case, REGS[(case["model"], sampler)], *PHILOX_KT, 2, True)


def _observe(eng, ctl, has_outputs):
    from test_kernel_sequence import _observe as observe
    return observe(eng, ctl, has_outputs)


def _sysnames(eng, ctl):
    # Robust's system 0 is the nominal one (robust_mppi_controller.cu:637)
    return (["nominal_sys", "real_sys"] if ctl == "robust" else ["real_sys", "nominal_sys"])[:eng.num_systems]


class _Run:
    """one scenario of one case: the oracle's call, and every handle created for it (closed by close())"""

    def __init__(self, case, name, K, T, tsallis=False, noise=None):
        self.case, self.name, self.K, self.T, self.tsallis = case, name, K, T, tsallis
        self.sc = scenario(name, case, K, T)
        self.noise = self.sc["noise"] if noise is None else noise
        self.ctl = case["controller"]
        self.tag = "%s %s K=%d T=%d%s" % (case["id"], name, K, T, " tsallis" if tsallis else "")
        self.handles = []  # (role, engine, streamed)
        self.cfg = self.orc = self.rob = None

    def add(self, role, env=None, reference_order=False, streamed=False, num_iters=None):
        sc = self.sc if num_iters is None else dict(self.sc, num_iters=num_iters)
        cfg, eng, orc, rob = scenario_handles(self.case, sc, self.K, self.T, env=env)
        self.handles.append((role, eng, streamed))
        if self.orc is None:
            self.cfg, self.orc, self.rob = cfg, orc, rob
            if self.tsallis:
                orc.set_colored_mppi_params(TSALLIS[0], TSALLIS[1], None, False, 1)
        if reference_order:
            eng.setReductionMode(m.MPPI_REDUCTION_REFERENCE_ORDER)
        if self.tsallis:
            eng.setColoredMPPIParams(gamma=TSALLIS[0], r_exp=TSALLIS[1])
        return eng

    def call_engine(self, eng):
        """one computeControl; Robust MPPI: its first cycle (no candidates yet) and the gains before it"""
        x0 = self.cfg["x0"]
        if self.sc["philox"]:
            eng.setSeed(PHILOX_SEED)
        else:
            eng.injectNoise(self.noise)
        if self.ctl == "robust":
            eng.updateImportanceSamplingControl(x0, 1)
            eng.setFeedbackGains(robust_gains(self.T, eng.STATE_DIM, eng.CONTROL_DIM))
        eng.computeControl(x0, 1)

    def call_oracle(self, num_iters=None):
        x0, orc, noise = self.cfg["x0"], self.orc, self.noise
        if num_iters is not None:
            noise = noise[:num_iters]
        if self.ctl == "colored":
            orc.colored_compute_control(x0, 1, noise, *self.cfg["colored"])
        elif self.ctl == "robust":
            self.rob.update_importance_sampling(x0, 1, None)
            self.rob.set_gains(robust_gains(self.T, orc.S, orc.C))
            self.rob.compute_control(x0, 1, noise)
        elif self.ctl == "tube":
            orc.tube_compute_control(x0, 1, noise)
        else:
            orc.vanilla_compute_control(x0, 1, noise)

    def close(self):
        for _, e, _ in self.handles:
            e.close()


def _check_against_oracle(run, eng, tag):
    """the reference-order handle: control and nominal control within U_TOL, baselines exact, normalisers 1e-6 relative, Tube
    nominal_state_used"""
    ctl, orc = run.ctl, run.orc
    du = float(np.abs(eng.getControlSeq() - orc.control()).max())
    assert du <= U_TOL, "%s: control differs from the oracle by %g" % (tag, du)
    if ctl in ("tube", "robust"):
        dn = float(np.abs(eng.getNominalControlSeq() - orc.nominal_control()).max())
        assert dn <= U_TOL, "%s: nominal control differs from the oracle by %g" % (tag, dn)
    st, ost = eng.getStats(), orc.stats()
    for z, name in enumerate(_sysnames(eng, ctl)):
        s = stats_of(st, name)
        assert s["baseline"] == ost["baseline"][z], "%s: %s baseline %r, oracle %r" % (tag, name, s["baseline"], ost["baseline"][z])
        rn = abs(s["normalizer"] - ost["normalizer"][z]) / abs(ost["normalizer"][z])
        assert rn <= NORM_RTOL_ORACLE, "%s: %s normaliser %g relative from the oracle" % (tag, name, rn)
    if ctl == "tube":
        assert st.nominal_state_used == ost["nominal_state_used"], "%s: nominal_state_used %d, oracle %d" % (
            tag, st.nominal_state_used, ost["nominal_state_used"])


def _check_float64(run, eng, tag, worst):
    """u* against the +inf-aware float64 softmin of the handle's OWN dumped costs and samples (SOFTMIN_RTOL as
    test_kernel_sequence._check_handle applies it), every statistic within stats64_inf's bound, and the scenario's exact
    consequences"""
    ctl, name, lam = run.ctl, run.name, run.cfg["lambda_"]
    costs, u_opt, v = eng.getSampledCostSeq(), eng.getOptimalControlSeq(), eng.getSampledControls()
    st = eng.getStats()
    for z, sysname in enumerate(_sysnames(eng, ctl)):
        c = costs[z]
        takeover = ctl == "tube" and z == 1 and st.nominal_state_used == 0
        if takeover:
            # tubeSelectKernel: the actual system won the pass, the nominal mean IS the actual one
            assert bits_equal(u_opt[1], u_opt[0], nan_equal=True), "%s: nominal u* after a take-over" % tag
        else:
            want = softmin64_inf(c, v[z], lam)
            err = float(np.abs(u_opt[z] - want).max())
            bound = SOFTMIN_RTOL * max(1.0, float(np.abs(want).max()))
            worst["u"] = max(worst.get("u", 0.0), err / bound)
            assert err <= bound, "%s: system %d u* is %g from the float64 softmin of its own samples (bound %g)" % (tag, z, err, bound)
        want, bound = stats64_inf(c, lam)
        got = stats_of(st, sysname)
        for k in STAT_KEYS:
            e = abs(got[k] - want[k])
            assert np.isfinite(bound[k]), (tag, k)
            if bound[k] > 0:
                worst[k] = max(worst.get(k, 0.0), float(e / bound[k]))
            assert e <= bound[k], "%s: %s %s = %r, float64 %r (bound %g)" % (tag, sysname, k, got[k], want[k], bound[k])
        # ---- exact consequences
        if name == "one_finite":
            k1 = int(np.flatnonzero(np.isfinite(c))[0])
            assert got["normalizer"] == 1.0, "%s: %s normaliser %r with one finite cost" % (tag, sysname, got["normalizer"])
            if not takeover:
                assert bits_equal(u_opt[z], v[z][k1]), "%s: system %d u* is not the sample of the one finite rollout %d" % (tag, z, k1)
        elif name == "all_tied":
            tied = c.view(np.uint32) == c[1].view(np.uint32)
            c64 = c.astype(np.float64)
            w = np.exp(-(c64 - c64.min()) / lam)
            expect = int(tied.sum()) * w[1] + w[~tied].sum()
            assert abs(got["normalizer"] - expect) <= bound["normalizer"], "%s: %s normaliser %r, %d tied rollouts give %r" % (
                tag, sysname, got["normalizer"], int(tied.sum()), expect)
        elif name == "tied_min":
            n = int((c.view(np.uint32) == c[np.argmin(c)].view(np.uint32)).sum())
            assert got["normalizer"] >= n, "%s: %s normaliser %r below the tie count %d" % (tag, sysname, got["normalizer"], n)


def _stats_bits(eng, ctl):
    st = eng.getStats()
    return np.array([list(stats_of(st, n).values()) for n in _sysnames(eng, ctl)], np.float32)


def _run_scenario(case, name, K, T, tsallis=False):
    run = _Run(case, name, K, T, tsallis)
    ctl = case["controller"]
    streamed = _streams(case, name)
    worst = {}
    try:
        run.add("reference-order", reference_order=True)
        run.add("fused, streamed" if streamed else "fused", streamed=streamed)
        if streamed:
            run.add("fused, two-launch", env=dict(MPPI_AMD_NO_STREAM_MERGE="1"))
        if ctl == "vanilla":
            run.add("fused, no merging control phase", env=dict(MPPI_AMD_NO_MERGE_CONTROL="1"), streamed=streamed)
        run.call_oracle()
        ocosts = run.orc.costs()
        for i, (role, eng, st) in enumerate(run.handles):
            tag = "%s [%s]" % (run.tag, role)
            run.call_engine(eng)
            check_form(case, eng, tag, streamed=st)
            # the fused handles start their 2nd iteration from a u* that differs from the oracle's by rounding: their costs are
            # the oracle's bit for bit in a one-iteration call only (tests/test_kernel_sequence.py)
            if i == 0 or run.sc["num_iters"] == 1:
                assert bits_equal(eng.getSampledCostSeq(), ocosts), "%s: costs differ from the oracle's (+inf at %d / %d rollouts)" % (
                    tag, int(np.isposinf(eng.getSampledCostSeq()).sum()), int(np.isposinf(ocosts).sum()))
            if i == 0:
                _check_against_oracle(run, eng, tag)
            elif tsallis:
                du = float(np.abs(eng.getControlSeq() - run.orc.control()).max())
                assert du <= U_TOL, "%s: control differs from the oracle by %g" % (tag, du)
            if not tsallis:  # (Tsallis weights are not the softmin's: held to the oracle alone)
                _check_float64(run, eng, tag, worst)
        # ---- the streamed merge against the two-launch twin, the merging control phase against its twin: bit for bit
        by_role = {r: e for r, e, _ in run.handles}
        pairs = [("fused, streamed", "fused, two-launch")] if streamed else []
        if ctl == "vanilla":
            pairs.append(("fused, streamed" if streamed else "fused", "fused, no merging control phase"))
        for a, b in pairs:
            oa, ob = _observe(by_role[a], ctl, by_role[a].OUTPUT_DIM > 0), _observe(by_role[b], ctl, by_role[b].OUTPUT_DIM > 0)
            for k in oa:
                assert bits_equal(oa[k], ob[k], nan_equal=True), "%s: %s of [%s] differs from [%s]" % (run.tag, k, a, b)
        # ---- weight zero means no influence: the crash rows' second channel * 1e3 changes not one bit
        if name in ZERO_WEIGHT_RERUN and not tsallis:
            again = _Run(case, name, K, T, noise=scale_second_channel(run.sc["noise"], run.sc["rows"], run.sc["colored"]))
            try:
                for (role, eng, _), ref in zip(run.handles[:2], (True, False)):
                    e2 = again.add(role, reference_order=ref)
                    again.call_engine(e2)
                    tag = "%s [%s]" % (run.tag, role)
                    assert bits_equal(e2.getOptimalControlSeq(), eng.getOptimalControlSeq()), "%s: u* changed with the zero-weight rollouts' samples" % tag
                    assert bits_equal(_stats_bits(e2, ctl), _stats_bits(eng, ctl)), "%s: statistics changed with the zero-weight rollouts' samples" % tag
            finally:
                again.close()
        print("softmin error / bound  %s: %s" % (run.tag, "  ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    finally:
        run.close()


def _run_all_inf(case, name, K, T, tsallis=False):
    """nothing has weight: MPPI_ERR_NAN, the dumped costs all +inf and the oracle's bits, baseline +inf, close() returns — on
    the first iteration; where the merge streams, a two-iteration handle merges the all-+inf records in its second launch.
    Nothing else is asserted about the NaN result.

    A Vanilla handle used to return MPPI_OK here with a control of -3.4028235e+38 in every entry (u* NaN, baseline +inf): its
    control phase clamps to the default ranges (+-FLT_MAX) with fminf(fmaxf(lo, u), hi), which drops the NaN.  The host now
    reads "nothing has weight" off the statistics that travel with the control (engine_controllers.hip: nothingHasWeight)."""
    run = _Run(case, name, K, T, tsallis)
    ctl = case["controller"]
    try:
        run.add("reference-order", reference_order=True, num_iters=1)
        run.add("fused", num_iters=1)
        if _streams(case, name):
            run.add("fused, streamed", streamed=True)
        run.call_oracle(num_iters=1)
        ocosts = run.orc.costs()
        assert np.isposinf(ocosts).all(), run.tag
        for role, eng, st in run.handles:
            tag = "%s [%s]" % (run.tag, role)
            status = m.MPPI_OK
            try:
                run.call_engine(eng)
            except m.MPPIError as e:
                status = e.status
            assert status == m.MPPI_ERR_NAN, "%s: computeControl returned status %d, u* %s, control %s, baselines %s" % (
                tag, status, eng.getOptimalControlSeq().reshape(-1)[:4], eng.getControlSeq().reshape(-1)[:4], _stats_bits(eng, ctl)[:, 0])
            check_form(case, eng, tag, streamed=st)
            if not st:
                assert bits_equal(eng.getSampledCostSeq(), ocosts), "%s: the dumped costs are not all +inf" % tag
                assert np.isposinf(_stats_bits(eng, ctl)[:, 0]).all(), "%s: baselines %s" % (tag, _stats_bits(eng, ctl)[:, 0])
    finally:
        run.close()  # (returns)
    # a handle created afterwards in the same process is a healthy one
    _run_scenario(case, "mixed_inf", *INJECTED_KT)


SCENARIO_PARAMS = [(c, n) for c in CASES for n in INJECTED + PHILOX]


@pytest.mark.gpu
@pytest.mark.parametrize("case,name", SCENARIO_PARAMS, ids=["%s-%s" % (c["id"], n) for c, n in SCENARIO_PARAMS])
def test_softmin_edges(gpu, case, name):
    for K, T in shapes_of(name, case["controller"], _record_edge(case)):
        (_run_all_inf if name in ALL_INF else _run_scenario)(case, name, K, T)


TSALLIS_PARAMS = [(c, n) for c in CASES if c["controller"] == "colored" for n in TSALLIS_SCENARIOS]


@pytest.mark.gpu
@pytest.mark.parametrize("case,name", TSALLIS_PARAMS, ids=["%s-%s" % (c["id"], n) for c, n in TSALLIS_PARAMS])
def test_tsallis_weights_at_infinite_costs(gpu, case, name):
    """tsallisWeightsKernel relies on `inf < gamma` being false: a +inf cost has weight 0 there too"""
    (_run_all_inf if name in ALL_INF else _run_scenario)(case, name, *INJECTED_KT, tsallis=True)


# ------------------------------------------------------------------ GPU: the merge on written records -------------------
def _floored_bounds(rec_z, TC, lam32, K):
    """_merge_reference's bounds with d_b s_b replaced by max(d_b s_b, 2^-126).  In the band (88, 103) lambda the true scale
    factor is below 2^-126, the smallest normal fp32 number: whatever the engine holds for it — a subnormal, a flush to zero,
    the smallest normal number — is within 2^-126 of it ABSOLUTELY, which no relative d_b expresses.  Derived, not measured.
    The floor enters every place d_b s_b does: sum_b |U_b[j]| (..) / eta, and rel_eta = sum_b eta_b (..) / eta."""
    ref, bound, vals, bounds = _merge_reference(rec_z, TC, lam32, K)
    u = UNIT
    W = rec_z.shape[0]
    r = rec_z.astype(np.float64)
    U, rho, eta_b, eta2_b = r[:, :TC], r[:, TC], r[:, TC + 1], r[:, TC + 2]
    lam = float(lam32)
    x = (rho - rho.min()) / lam
    s = np.exp(-x)
    d = 3 * u * x + 4 * u
    ds = np.maximum(d * s, SUBNORMAL_FLOOR)
    eta = vals["normalizer"]
    rel_eta = (eta_b * ds).sum() / eta
    bound = (np.abs(U) * (ds[:, None] + s[:, None] * W * u)).sum(0) / eta + np.abs(ref) * (rel_eta + 3 * u)
    eta2 = (s * s * eta2_b).sum()
    e1 = rel_eta + 3 * u
    e2 = (s * eta2_b * (2 * ds + s * u)).sum() / eta2 + 3 * u
    mean, mean2 = eta / K, eta2 / K
    var, mod = vals["free_energy_variance"], vals["free_energy_modified_variance"]
    q = var / (mean * np.sqrt(K))
    d_fe = lam * e1 + 8 * u * (lam * abs(np.log(mean)) + abs(vals["baseline"]))
    d_var = lam * (e2 * mean2 + (2 * e1 + u) * mean * mean) + 3 * u * abs(var)
    d_q = d_var / (mean * np.sqrt(K)) + abs(q) * (e1 + 6 * u)
    d_mod = lam * (1 + abs(q)) * d_q + 4 * u * abs(mod)
    bounds = dict(baseline=0.0, normalizer=SOFTMIN_RTOL * eta, free_energy_mean=d_fe,
                  free_energy_variance=d_var, free_energy_modified_variance=d_mod)
    return ref, bound, vals, bounds


def _edge_reference(kind, rec_z, TC, lam32, K):
    """float64 merge of one system's edge records -> (u*, bound, statistics, bounds).  A record with rho = +inf has scale 0 and
    U = eta = eta2 = 0: the merge is that of the other records (the K behind the statistics still counts its rollouts)"""
    if kind == "subnormal_band":
        return _floored_bounds(rec_z, TC, lam32, K)
    keep = np.isfinite(rec_z[:, TC])
    return _merge_reference(rec_z[keep], TC, lam32, K)


def test_edge_merge_inputs_are_what_they_claim():
    """CPU: the +inf records are the epilogue's (U = eta = eta2 = 0) at the first, a middle and the last position; the band set
    lies in (88, 103) lambda after the fp32 rounding of lambda and 1 / lambda, where test_merge_inputs_avoid_the_subnormal_
    scale_factors keeps the old sets out"""
    for _, model, D, C, T in MERGE_PROBLEMS:
        lam32 = np.float32(MERGE_LAMBDA[model])
        TC = T * C
        for W in MERGE_WORLDS:
            for i, kind in enumerate(EDGE_MERGE_SETS):
                rec = edge_merge_records(kind, W, D, TC, float(lam32), seed=2000 * W + 10 * TC + i)
                inf = np.isposinf(rec[:, :, TC])
                assert (inf == inf[:, :1]).all() and not np.isnan(rec).any()
                where = list(np.flatnonzero(inf[:, 0]))
                if kind == "subnormal_band":
                    assert not where
                    for z in range(D):
                        x = np.array([scale_arg32(rec[b, z, TC], rec[:, z, TC].min(), lam32) for b in range(W)])
                        assert x[0] == 0 and ((x[1:] > 88.0) & (x[1:] < 103.0)).all(), (model, W, x)
                        assert (np.exp(-_merge_x(rec, TC, lam32)[1:, z]) < SUBNORMAL_FLOOR).all()
                    continue
                assert where == {"inf_first": [0], "inf_middle": [W // 2], "inf_last": [W - 1],
                                 "inf_several": sorted({0, W // 2, W - 1} - {1}), "inf_all": list(range(W))}[kind], (kind, W)
                assert (rec[inf] == np.where(np.arange(TC + 4) == TC, np.inf, 0.0)).all(), kind
                assert len(where) < W or kind == "inf_all"


@pytest.mark.gpu
@pytest.mark.parametrize("problem", MERGE_PROBLEMS, ids=[p[0] for p in MERGE_PROBLEMS])
def test_gathered_merge_on_edge_records(gpu, problem):
    tag0, model, D, C, T = problem
    TC = T * C
    lam32 = np.float32(MERGE_LAMBDA[model])
    for W in MERGE_WORLDS:
        cfg = _merge_cfg(model, D, W, T)
        K = cfg["K"]
        eng = make_engine(cfg, tube=D == 2, rank=0, world_size=W)
        try:
            eng.uploadState(np.tile(cfg["x0"], (D, 1)))
            eng.iterationLocal()
            for i, kind in enumerate(EDGE_MERGE_SETS):
                tag = "%s world=%d %s" % (tag0, W, kind)
                rec = edge_merge_records(kind, W, D, TC, float(lam32), seed=2000 * W + 10 * TC + i)
                u, st = _merge_once(eng, rec, D)
                if kind == "inf_all":
                    assert np.isnan(u).all(), "%s: u* %s" % (tag, u)
                    assert all(s["baseline"] == np.inf for s in st), "%s: baselines %s" % (tag, [s["baseline"] for s in st])
                    # mergeScale's rule: an all-+inf record has the scale 0 (not exp(-(inf - inf) / lambda) = NaN), and with
                    # eta_b = 0 the normaliser is the exact sum of zeros: nothing has weight
                    assert all(s["normalizer"] == 0.0 for s in st), "%s: normalisers %s" % (tag, [s["normalizer"] for s in st])
                    continue
                worst = dict(u=0.0)
                for z in range(D):
                    ref, bound, vals, bounds = _edge_reference(kind, rec[:, z], TC, lam32, K)
                    err = np.abs(u[z].reshape(-1).astype(np.float64) - ref)
                    j = int(np.argmax(err / bound))
                    worst["u"] = max(worst["u"], float(err[j] / bound[j]))
                    assert (err <= bound).all(), "%s: system %d u*[%d] = %r, float64 merge %r: off by %g, bound %g" % (
                        tag, z, j, u[z].reshape(-1)[j], ref[j], err[j], bound[j])
                    for k in vals:
                        e = abs(st[z][k] - vals[k])
                        if bounds[k] > 0:
                            worst[k] = max(worst.get(k, 0.0), float(e / bounds[k]))
                        assert e <= bounds[k], "%s: system %d %s = %r, float64 %r (bound %g)" % (tag, z, k, st[z][k], vals[k], bounds[k])
                print("merge error / bound  %s: %s" % (tag, "  ".join("%s %.3f" % kv for kv in worst.items())))
        finally:
            eng.close()


# ------------------------------------------------------------------ GPU: the unfused operators --------------------------
OPERATOR_K = (1, 63, 1025, 10000)
OPERATOR_PATTERNS = ("some_inf", "one_finite", "all_inf", "tied_min", "all_equal", "beyond_104", "band_88_103")
OPERATOR_LAMBDA = 0.5


def operator_costs(pattern, K):
    rng = np.random.default_rng(K + len(pattern))
    lam = OPERATOR_LAMBDA
    c = rng.uniform(5.0, 5.0 + 10 * lam, K).astype(np.float32)
    k0 = K // 2
    c[k0] = 4.0  # the minimum
    if pattern == "some_inf":
        c[rng.random(K) < 0.4] = np.inf
        c[k0] = 4.0
    elif pattern == "one_finite":
        c[:] = np.inf
        c[k0] = 4.0
    elif pattern == "all_inf":
        c[:] = np.inf
    elif pattern == "tied_min":
        c[rng.integers(0, K, 5)] = 4.0
    elif pattern == "all_equal":
        c[:] = 4.0
    elif pattern == "beyond_104":
        far = np.arange(K) != k0
        c[far] = 4.0 + lam * rng.uniform(105.0, 1e4, K)[far].astype(np.float32)
    elif pattern == "band_88_103":
        far = np.arange(K) % 2 == 1
        c[far] = 4.0 + lam * rng.uniform(88.5, 102.5, K)[far].astype(np.float32)
        c[k0] = 4.0
    return c


def test_operator_patterns_are_what_they_claim():
    lam = OPERATOR_LAMBDA
    for K in OPERATOR_K:
        for p in OPERATOR_PATTERNS:
            c = operator_costs(p, K)
            assert c.shape == (K,) and not np.isnan(c).any()
            x = np.array([scale_arg32(v, c.min(), lam) for v in c[np.isfinite(c)]])
            if p == "all_inf":
                assert np.isposinf(c).all()
            elif p == "one_finite":
                assert int(np.isfinite(c).sum()) == 1
            elif p == "some_inf" and K >= 63:
                assert 0 < int(np.isposinf(c).sum()) < K
            elif p == "tied_min":
                assert int((c == c.min()).sum()) >= min(K, 2)
            elif p == "all_equal":
                assert (c == c[0]).all()
            elif p == "beyond_104":
                assert (np.sort(x)[1:] > 104.0).all()
            elif p == "band_88_103" and K > 1:
                band = (x > 88.0) & (x < 103.0)
                assert int(band.sum()) >= K // 2 - 1 and (band | (x < 12.5)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", OPERATOR_PATTERNS)
@pytest.mark.parametrize("K", OPERATOR_K)
def test_unfused_operators_at_edge_costs(gpu, K, pattern):
    """m.norm_exp / m.compute_weights / m.weighted_reduction keep the REFERENCE semantics: weights and baseline are the oracle's
    bit for bit (NaN == NaN: everything +inf gives NaN weights, exp(-(inf - inf) / lambda)); normaliser and u within the
    relative bounds of tests/test_gpu_ops.py"""
    lam = OPERATOR_LAMBDA
    lambda_inv = 1.0 / lam
    costs = operator_costs(pattern, K)
    base = po.baseline(costs)
    w_o = po.norm_exp(costs, lambda_inv, base)
    assert bits_equal(m.norm_exp(costs, lambda_inv, base), w_o, nan_equal=True), "norm_exp"
    w, b, eta = m.compute_weights(costs, lambda_inv)
    assert bits_equal([b], [base], nan_equal=True), (b, base)
    assert bits_equal(w, w_o, nan_equal=True), "compute_weights"
    eta_o = po.normalizer(w_o)
    if pattern == "all_inf":
        assert np.isnan(w_o).all() and np.isnan(eta) and np.isnan(eta_o)
        return
    assert abs(eta - eta_o) <= 1e-6 * eta_o, (eta, eta_o)
    rng = np.random.default_rng(K)
    v = rng.normal(5.0, 1.2, (K, 7, 2)).astype(np.float32)
    u_gpu = m.weighted_reduction(w_o, v, eta_o)
    u_cpu = po.weighted_reduction(w_o, v, eta_o, 64)
    assert np.abs(u_gpu - u_cpu).max() <= 1e-5 * np.abs(u_cpu).max(), np.abs(u_gpu - u_cpu).max()
