"""Every registered kernel form against the oracle with the sampler's options switched on.

tests/test_kernel_matrix.py and tests/test_kernel_sequence.py run every form on one sampler configuration: a zero
likelihood-ratio coefficient (GaussianDistribution::computeLikelihoodRatioCost then returns before it reads a mean or a sigma),
alpha = 0, std_dev_decay = 1, 1 % pure-noise rollouts, one sigma per control, noise shared by both systems and a zero initial
mean.  Here the same enumeration (build_cases / BUILDERS / _make of the kernel matrix: a new registration is covered without
touching this file) runs under two option sets, both with std_dev_decay = 0.9, alpha = 0.1, 25 % pure-noise rollouts and a
distinct non-zero likelihood-ratio coefficient per control:
  table        a time-specific sigma [D][T][C] that differs in every (d, t, c) while std_dev stays at the builder's value (a
               kernel that reads the wrong source fails), and — Tube, Robust — independent noise per distribution
               ([n][D][K][T][C] injected, Philox stream d in the generator mode);
  per-control  no table, std_dev [D][C] different for the two distributions and for every control, shared noise.
Colored handles run both sets without independent noise, which the engine refuses for them (asserted once).  Vanilla, Tube and
Colored handles start from a non-zero mean inside the control ranges; Robust MPPI keeps the kernel matrix's first-cycle
protocol (its nominal control starts at zero, the means of both its distributions are non-zero in the second iteration).

Shapes.  Injected noise at (K, T) = (65, 3), (200, 5), (1049, 9), Philox at (65, 17).  With 25 % pure-noise rollouts (exact in
fp32) the first pure-noise rollout is 49 (48.75: inside a wave), 150 (150.0 exactly: the equality edge of the reference's float
compare) and 787 (786.75: inside a block).  T = 5 is shorter than one replicated-lane sampling pass of 8 steps, T = 9 is one
pass and a tail, T = 17 two passes and a tail that ends inside a Philox quad for two controls.  The optimisation stride is 2
where T >= 5 (t < stride takes the mean) and 1 at T = 3.

Per (case, set, shape), one iteration in the default reduction: the launched form, sampled costs and dumped samples 0 ulp
against the oracle, u* (and the nominal u*) within 1e-5, and three float64 checks in numpy on the handle's own dumps that share
no code with the oracle:
  sample rule       v = clamp(rule(mean, decay^it sigma[d][t][c], eps, k, t)) within 2^-21 max(1, |m| + |sigma e|): four fp32
                    roundings (decay * sigma, sigma * e, the sum, and half an ulp of slack on the clamp bound) and one possible
                    fma contraction.  Not Robust (its dumped samples carry the feedback term).  Every registered plugin keeps the
                    base clamp, so SAMPLE_RULE_SKIP is empty; it may only ever name plugins with state-dependent constraints;
  likelihood ratio  a twin handle with a zero coefficient, the same mean and noise: S_coeff - S_0 against
                    (1/T) sum_t 0.5 lambda (1 - alpha) sum_j c_j mu_j (mu_j - 2 v_j) / sigma_j^2 from the dumped v, mu = 0 on
                    pure-noise rollouts, the undecayed sigma; bound (T + 4) 2^-23 (max(|S_coeff|, |S_0|) + sum_t |LR_t| / T):
                    the worst-case fp32 summation error of two T-term running sums plus the term's own roundings.  Robust:
                    the real system (row 1) — its mean is zero in the first iteration, so the term must vanish there; the
                    combined nominal cost also carries the feedback cost, which the coefficient scales too;
  softmin           u* against the float64 softmin of the handle's own costs and samples (SOFTMIN_RTOL of the kernel matrix).
                    Not Robust.

Per (case, set) at (200, 5) and (1049, 9), two iterations on two handles as in test_kernel_sequence.py: iteration 1 samples with
decay^1 around the merged non-zero mean.  The reference-order handle: costs 0 ulp, u* within 1e-5, baselines exact.  The default
fused handle: u* within 1e-5 of the oracle (or a measured drift in FUSED_DRIFT) and streamed_merge as expects_streamed_merge
says.  None of the shapes above lets the merge stream (T C % 4 != 0, and injected noise never streams), so the cases whose
fused handle can stream also run two Philox iterations at (200, 8): there the likelihood-ratio term reads its means from the LDS
row the sampler waves have just merged; the streamed handle is held to the oracle's u* and, bit for bit, to a two-launch twin.
"""
import functools
import glob
import os

import numpy as np
import pytest

import mppi_generic_amd as m
import pyoracle as po
from common import PHILOX_SEED, U_TOL, host_noise, host_spectrum, make_oracle
from kernel_forms import (BUILDERS, build_cases, check_against_oracle, check_form, compute_once, expects_streamed_merge,
                          make_handles, registrations)
from restate64 import (SOFTMIN_RTOL, bits_equal, constrain64, first_pure_rollout, likelihood_ratio64, likelihood_ratio_bound,
                       ranges32, sample_rule64, softmin64)

SETS = ("table", "per-control")
DECAY, ALPHA, PURE_PCT = 0.9, 0.1, 0.25
COEFF = (0.7, 0.3)
# models whose state cost is so large against lambda that COEFF's likelihood-ratio term stays below the share
# test_likelihood_ratio_share_and_restatements asks for (Cartpole 1.2e-4, the RACER models 2.1e-4 .. 4.5e-4 of the cost with
# COEFF itself): model -> factor on COEFF
COEFF_SCALE = dict({"cartpole": 20.0}, **{name: 8.0 for name in BUILDERS if name.startswith("racer_dubins")})
SIGMA_SETS = ((0.8, 1.3), (1.15, 0.7))  # per-control set: factor on the builder's std_dev, [distribution][control]
KT_INJECTED = [(65, 3), (200, 5), (1049, 9)]
KT_PHILOX = (65, 17)
KT_TWO_ITERS = [(200, 5), (1049, 9)]
KT_STREAMED = (200, 8)  # T C % 4 == 0 for one and two controls: the fused 64x1x1 pipeline streams its merge (Philox only)

# plugins whose enforceConstraints depends on the state: constrain64 cannot restate their clamp -> model name: reason.  No
# registered plugin declares CONSTRAINTS_DEPEND_ON_STATE (test_coverage holds the list to those that do).
SAMPLE_RULE_SKIP = {}

# Default (fused) handles whose control drifts past U_TOL from the oracle over the two iterations while the reference-order
# handle of the same run is exact: (case id, set, (K, T)) -> the difference measured against the oracle times 1.25.
# All eight are Tube handles of the elevation-map RACER models under the table set (independent noise per distribution) at
# (1049, 9): the fused merge sums the weighted samples in another order than the reference, iteration 1 samples around that
# u*, and the difference grows through the dynamics — as in test_kernel_sequence.FUSED_DRIFT.
_K9 = (1049, 9)
FUSED_DRIFT = {
    ("racer_dubins_elevation-tube-fused64x4x2", "table", _K9): 1.93e-5,                    # measured 1.541e-5, times 1.25
    ("racer_dubins_elevation-tube-fused64x1x2", "table", _K9): 1.93e-5,                    # measured 1.541e-5, times 1.25
    ("racer_dubins_elevation-tube-pipeline64x1x2", "table", _K9): 1.93e-5,                 # measured 1.541e-5, times 1.25
    ("racer_dubins_elevation-tube-fused64x4x2-hbm", "table", _K9): 1.93e-5,                # measured 1.541e-5, times 1.25
    ("racer_dubins_elevation-tube-pipeline64x1x2-hbm", "table", _K9): 1.93e-5,             # measured 1.541e-5, times 1.25
    ("racer_dubins_elevation_lstm_steering-tube-fused64x4x2", "table", _K9): 1.86e-5,      # measured 1.487e-5, times 1.25
    ("racer_dubins_elevation_lstm_steering-tube-fused64x1x2", "table", _K9): 1.86e-5,      # measured 1.487e-5, times 1.25
    ("racer_dubins_elevation_lstm_steering-tube-fused64x4x2-hbm", "table", _K9): 1.86e-5,  # measured 1.487e-5, times 1.25
}


def stride_of(T):
    return 2 if T >= 5 else 1


@functools.lru_cache(maxsize=None)
def _model_info(model):
    cfg = BUILDERS[model](1, 1, 1)
    C = len(cfg["control_cost_coeff"])
    return dict(C=C, std_dev=np.asarray(cfg["std_dev"], np.float64).reshape(-1)[:C], ranges=ranges32(cfg, C))


class Options:
    """everything one (model, controller, option set, K, T) run is configured with, as numpy arrays"""

    def __init__(self, model, controller, set_name, K, T, zero_coeff=False):
        info = _model_info(model)
        C = self.C = info["C"]
        D = self.D = 2 if controller in ("tube", "robust") else 1
        self.model, self.controller, self.set_name, self.K, self.T = model, controller, set_name, K, T
        self.stride = stride_of(T)
        self.coeff = np.zeros(C) if zero_coeff else COEFF_SCALE.get(model, 1.0) * np.asarray(COEFF[:C], np.float64)
        base = info["std_dev"]
        self.overlay = dict(alpha=ALPHA, pure_pct=PURE_PCT, decay=DECAY, control_cost_coeff=[float(c) for c in self.coeff])
        self.table = None
        if set_name == "table":
            # base sigma times a factor in [0.7, 1.3) that differs in every (d, t, c): multiples of the golden ratio mod 1
            idx = np.arange(D * T * C, dtype=np.float64).reshape(D, T, C)
            self.table = (base[None, None, :] * (0.7 + 0.6 * np.mod((idx + 1.0) * 0.6180339887498949, 1.0))).astype(np.float32)
            self.sigma = self.table.astype(np.float64)
        else:
            sd = np.stack([base * np.asarray(SIGMA_SETS[d][:C]) for d in range(D)]).astype(np.float32)
            self.overlay["std_dev"] = [float(s) for s in sd.reshape(-1)]
            self.sigma = np.repeat(sd.astype(np.float64)[:, None, :], T, 1)
        self.independent = set_name == "table" and controller in ("tube", "robust")
        # initial mean: a third of the way from the centre of the control range to its bounds (no range: one builder sigma)
        lo, hi = info["ranges"]
        ranged = np.isfinite(lo) & np.isfinite(hi)
        centre = np.where(ranged, 0.5 * (np.where(ranged, lo, 0.0) + np.where(ranged, hi, 0.0)), 0.0)
        half = np.where(ranged, 0.5 * (np.where(ranged, hi, 0.0) - np.where(ranged, lo, 0.0)), base)
        t = np.arange(T, dtype=np.float64)[:, None]
        c = np.arange(C, dtype=np.float64)[None, :]
        self.mean = (centre + 0.35 * half * np.sin(0.9 * t + 1.7 * c + 0.4)).astype(np.float32)
        if controller == "robust":
            self.mean = np.zeros((T, C), np.float32)

    def apply(self, eng=None, orc=None):
        """the options that are not part of the cfg, on an engine handle and / or an oracle"""
        if eng is not None:
            if self.table is not None:
                eng.setTimeSpecificStdDev(self.table)
            if self.independent:
                eng.setIndependentNoise(True)
            if self.controller != "robust":
                eng.updateImportanceSampler(self.mean)
        if orc is not None:
            orc.set_time_specific_std_dev(self.table)
            orc.set_independent_noise(self.independent)
            if self.controller != "robust":
                orc.set_nominal_control(self.mean)

    def noise(self, n_iters, philox):
        """(what the engine is injected with or None, what the oracle is handed): n_iters generations from generation 0"""
        K, T, C, D = self.K, self.T, self.C, self.D
        if self.controller == "colored":
            if philox:
                return None, np.stack([po.philox_spectrum(PHILOX_SEED, g, K, T, C) for g in range(n_iters)])
            z = host_spectrum(n_iters, K, T, C, seed=K + T)
            return z, z
        if philox:
            if self.independent:
                return None, np.stack([np.stack([po.philox_normal(PHILOX_SEED, g, K, T, C, stream=d) for d in range(D)])
                                       for g in range(n_iters)])
            return None, np.stack([po.philox_normal(PHILOX_SEED, g, K, T, C) for g in range(n_iters)])
        if self.independent:
            eps = np.random.Generator(np.random.Philox(K + T)).standard_normal((n_iters, D, K, T, C), dtype=np.float32)
        else:
            eps = host_noise(n_iters, K, T, C, seed=K + T)
        return eps, eps

    def eps_of_system(self, eps, z, colored_params=None):
        """the time-domain noise [K][T][C] system z shapes in iteration 0"""
        if self.controller == "colored":
            exps, decay, fmin = colored_params
            return po.colored_noise(eps[0], exps, decay, fmin, offset_t=self.stride, flavour="engine")
        return eps[0][z] if self.independent else eps[0]


# ------------------------------------------------------------------ cases -----------------------------------------------
def option_cases():
    regs = {(n, s): d for n, s, d in registrations()}
    out = []
    for case in build_cases():
        if case["refuse"]:
            continue
        sampler = m.MPPI_SAMPLER_COLORED if case["controller"] == "colored" else m.MPPI_SAMPLER_GAUSSIAN
        d = regs[(case["model"], sampler)]
        C = _model_info(case["model"])["C"]
        out.append(dict(case, C=C, streams=expects_streamed_merge(case, d, *KT_STREAMED, C, True)))
    return out


CASES = option_cases()
# as enumerated when this module is imported: tests that run earlier in a session may register models of their own
# (plugins, templated examples), which are theirs to hold to the oracle
REGISTRATIONS = registrations()


# ------------------------------------------------------------------ CPU ------------------------------------------------
def _oracle_run(model, controller, set_name, K, T, zero_coeff=False):
    """the oracle alone, one iteration with injected noise: (options, cfg, costs [D][K], clamped samples [D][K][T][C], eps)"""
    opt = Options(model, controller, set_name, K, T, zero_coeff)
    cfg = BUILDERS[model](K, T, opt.D)
    cfg["D"] = opt.D
    cfg["num_iters"] = 1
    cfg.update(opt.overlay)
    orc = make_oracle(cfg)
    opt.apply(orc=orc)
    _, eps = opt.noise(1, False)
    (orc.tube_compute_control if controller == "tube" else orc.vanilla_compute_control)(cfg["x0"], opt.stride, eps)
    return opt, cfg, orc.costs(), orc.samples(), eps


@pytest.mark.parametrize("set_name", SETS)
@pytest.mark.parametrize("model", sorted(BUILDERS))
def test_likelihood_ratio_share_and_restatements(model, set_name):
    """conditions on the inputs, on the oracle alone at (200, 5): the likelihood-ratio term is a visible share of every
    model's costs (median over the rollouts of |S_coeff - S_0| / |S_0| >= 1e-3 — else a kernel that drops or garbles the term
    would pass a 1e-5 comparison of u*), the mean is non-zero, and the two float64 restatements hold against the oracle
    within the bounds the GPU test uses"""
    K, T = 200, 5
    for controller in ("vanilla", "tube"):
        opt, cfg, s_coeff, v, eps = _oracle_run(model, controller, set_name, K, T)
        _, _, s_zero, v0, _ = _oracle_run(model, controller, set_name, K, T, zero_coeff=True)
        tag = "%s %s %s" % (model, controller, set_name)
        assert np.array_equal(v, v0), tag
        assert np.isfinite(s_coeff).all() and np.isfinite(s_zero).all(), tag
        fp = first_pure_rollout(K, PURE_PCT)
        assert float(np.abs(opt.mean[opt.stride:]).max()) > 0 and float(np.abs(opt.mean).min()) > 0, tag
        lo_hi = ranges32(cfg, opt.C)
        assert (opt.mean.astype(np.float64) > lo_hi[0]).all() and (opt.mean.astype(np.float64) < lo_hi[1]).all(), tag
        for z in range(opt.D):
            share = float(np.median(np.abs(s_coeff[z] - s_zero[z]) / np.abs(s_zero[z])))
            assert share >= 1e-3, "%s system %d: the likelihood-ratio term is %g of the cost (median)" % (tag, z, share)
            want, bound = sample_rule64(opt.mean, opt.sigma[z], opt.eps_of_system(eps, z), opt.stride, fp, lo_hi, DECAY)
            err = np.abs(v[z].astype(np.float64) - want)
            assert (err <= bound).all(), "%s system %d: sample rule off by %g" % (tag, z, float((err - bound).max()))
            if model not in SAMPLE_RULE_SKIP:
                assert np.array_equal(constrain64(v[z].reshape(-1, opt.C), lo_hi), v[z].reshape(-1, opt.C)), tag
            lr, lr_abs = likelihood_ratio64(v[z], opt.mean, opt.sigma[z], opt.coeff, fp, cfg["lambda_"], ALPHA)
            err = np.abs((s_coeff[z].astype(np.float64) - s_zero[z].astype(np.float64)) - lr)
            bound = likelihood_ratio_bound(T, s_coeff[z], s_zero[z], lr_abs)
            assert (err <= bound).all(), "%s system %d: likelihood ratio off by %g (bound %g)" % (
                tag, z, float(err.max()), float(bound[np.argmax(err - bound)]))


def test_option_sets_differ_where_a_wrong_source_must_show():
    """the table differs in every (d, t, c) and from the builder's std_dev; the per-control sigmas differ between the
    distributions and the controls; the coefficients are distinct and non-zero"""
    for model in sorted(BUILDERS):
        base = _model_info(model)["std_dev"]
        a = Options(model, "tube", "table", 65, 17)
        assert a.table.shape == (2, 17, a.C) and (a.table > 0).all()
        rel = a.table / base.astype(np.float32)
        assert np.unique(rel).size == rel.size and (np.abs(rel - 1.0) > 1e-4).all(), model
        assert "std_dev" not in a.overlay and a.independent
        b = Options(model, "tube", "per-control", 65, 17)
        rel = np.asarray(b.overlay["std_dev"]).reshape(2, b.C) / base
        assert np.unique(np.round(rel, 6)).size == rel.size and b.table is None and not b.independent, model
        assert (a.coeff != 0).all() and np.unique(a.coeff).size == a.C
        assert not Options(model, "colored", "table", 65, 17).independent
        assert not np.any(Options(model, "robust", "table", 65, 17).mean)


def test_pure_noise_boundaries():
    """(1 - 0.25) K in fp32: 48.75, 150.0 (the equality edge: rollout 150 is pure) and 786.75 — against the oracle's isPureNoise"""
    assert [first_pure_rollout(K, PURE_PCT) for K, _ in KT_INJECTED] == [49, 150, 787]
    assert first_pure_rollout(KT_PHILOX[0], PURE_PCT) == 49
    assert np.float32(PURE_PCT) == PURE_PCT and (np.float32(1) - np.float32(PURE_PCT)) * np.float32(200) == np.float32(150)
    for K, T in KT_INJECTED:
        orc = po.Oracle("cartpole", K, T, 1)
        orc.set_sampler([1.0], [0.0], PURE_PCT, 1.0)
        v = orc.set_gaussian_controls(np.ones((1, T, 1), np.float32), np.zeros((K, T, 1), np.float32), 0, 0)
        # zero noise around a mean of one: a rollout that uses the mean holds 1, a pure-noise rollout 0; rollout 0 is the mean
        pure = v[0, :, T - 1, 0] == 0
        fp = first_pure_rollout(K, PURE_PCT)
        assert not pure[:fp].any() and pure[fp:].all(), (K, fp)


def test_coverage():
    """every registration has a runnable case here, with the kernel matrix's ids; nothing is skipped on the GPU except through
    SAMPLE_RULE_SKIP, which may hold at most the plugins that declare state-dependent constraints"""
    cases = CASES
    matrix = [c for c in build_cases() if not c["refuse"] and c["model"] in BUILDERS]
    assert [c["id"] for c in cases] == [c["id"] for c in matrix]
    assert {r[0] for r in REGISTRATIONS} == set(BUILDERS)
    for name, sampler, d in REGISTRATIONS:
        prefix = name + ("[colored]" if sampler else "") + "-"
        assert [c for c in cases if c["id"].startswith(prefix)], "registration %s has no runnable case" % prefix
        if d["pipeline"] and d["streamed_merge"]:
            assert [c for c in cases if c["id"].startswith(prefix) and c["streams"]], \
                "registration %s streams its merge but no case here runs the streamed iteration" % prefix
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    declaring = 0
    for path in glob.glob(os.path.join(inc, "**", "*.hpp"), recursive=True) + glob.glob(os.path.join(inc, "**", "*.cuh"),
                                                                                      recursive=True):
        with open(path, errors="replace") as f:
            declaring += f.read().replace(" ", "").count("CONSTRAINTS_DEPEND_ON_STATE=true")
    assert set(SAMPLE_RULE_SKIP) <= set(BUILDERS) and len(SAMPLE_RULE_SKIP) <= declaring
    for key in FUSED_DRIFT:
        assert key[0] in {c["id"] for c in cases} and key[1] in SETS and key[2] in KT_TWO_ITERS + [KT_STREAMED], key


# ------------------------------------------------------------------ GPU ------------------------------------------------
def _compute(case, opt, cfg, engines, orc, rob, philox, n_iters):
    """one computeControl of n_iters iterations on every engine and on the oracle, from the same noise; returns that noise"""
    _, eps = opt.noise(n_iters, philox)
    compute_once(case, engines, orc, rob, cfg, opt.stride, eps, philox, PHILOX_SEED)
    return eps


def _run_one_iteration(case, set_name, K, T, philox):
    ctl = case["controller"]
    tag = "%s [%s] K=%d T=%d%s" % (case["id"], set_name, K, T, " philox" if philox else "")
    opt = Options(case["model"], ctl, set_name, K, T)
    opt0 = Options(case["model"], ctl, set_name, K, T, zero_coeff=True)
    cfg, eng, orc, rob = make_handles(case, K, T, overlay=opt.overlay)
    cfg0, twin, orc0, rob0 = make_handles(case, K, T, overlay=opt0.overlay)
    try:
        opt.apply(eng, orc)
        opt0.apply(twin, orc0)
        eps = _compute(case, opt, cfg, [eng], orc, rob, philox, 1)
        _compute(case, opt0, cfg0, [twin], orc0, rob0, philox, 1)
        check_form(case, eng, tag)
        check_form(case, twin, tag + " [zero coefficient]")
        du = check_against_oracle(case, eng, orc, tag, samples_exact=True)
        print("FIGURE %s: control differs from the oracle by %.3e" % (tag, du))
        assert du <= U_TOL, "%s: u* (or the nominal u*) differs from the oracle by %g" % (tag, du)

        # ---- float64, from the handle's own dumps
        costs, v, u_opt = eng.getSampledCostSeq(), eng.getSampledControls(), eng.getOptimalControlSeq()
        costs0, v0 = twin.getSampledCostSeq(), twin.getSampledControls()
        lo_hi = ranges32(cfg, opt.C)
        fp = first_pure_rollout(K, PURE_PCT)
        lam = cfg["lambda_"]
        for z in range(eng.num_systems):
            if ctl != "robust" and case["model"] not in SAMPLE_RULE_SKIP:
                want, bound = sample_rule64(opt.mean, opt.sigma[z], opt.eps_of_system(eps, z, cfg.get("colored")), opt.stride,
                                            fp, lo_hi, DECAY)
                err = np.abs(v[z].astype(np.float64) - want)
                assert (err <= bound).all(), "%s: system %d sample (k, t, c) = %s is %g from the float64 rule (bound %g)" % (
                    tag, z, np.unravel_index(np.argmax(err - bound), err.shape), float(err.flat[np.argmax(err - bound)]),
                    float(bound.flat[np.argmax(err - bound)]))
            if ctl != "robust" or z == 1:
                assert bits_equal(v[z], v0[z]), "%s: system %d samples depend on the likelihood-ratio coefficient" % (tag, z)
                lr, lr_abs = likelihood_ratio64(v[z], opt.mean, opt.sigma[z], opt.coeff, fp, lam, ALPHA)
                err = np.abs((costs[z].astype(np.float64) - costs0[z].astype(np.float64)) - lr)
                bound = likelihood_ratio_bound(T, costs[z], costs0[z], lr_abs)
                k = int(np.argmax(err - bound))
                assert (err <= bound).all(), "%s: system %d rollout %d: S_coeff - S_0 is %g from the float64 likelihood-ratio " \
                    "term %g (bound %g)" % (tag, z, k, float(err[k]), float(lr[k]), float(bound[k]))
            if ctl != "robust":
                if ctl == "tube" and z == 1 and eng.getStats().nominal_state_used == 0:
                    # tubeSelectKernel: the actual system won the pass, the nominal mean IS the actual one
                    assert bits_equal(u_opt[1], u_opt[0]), "%s: nominal u* after a take-over" % tag
                    continue
                want = softmin64(costs[z], v[z], lam)
                err = float(np.abs(u_opt[z] - want).max())
                bound = SOFTMIN_RTOL * max(1.0, float(np.abs(want).max()))
                assert err <= bound, "%s: system %d u* is %g from the float64 softmin of its own samples" % (tag, z, err)
    finally:
        eng.close()
        twin.close()


def _run_two_iterations(case, set_name, K, T, philox):
    """reference-order handle and default fused handle (and, where that one streams its merge, a two-launch twin) through two
    iterations: iteration 1 shapes with decay^1 around the merged mean of iteration 0"""
    ctl = case["controller"]
    tag = "%s [%s] K=%d T=%d%s two iterations" % (case["id"], set_name, K, T, " philox" if philox else "")
    streams = bool(philox and case["streams"] and (K, T) == KT_STREAMED)
    opt = Options(case["model"], ctl, set_name, K, T)
    cfg, exact, orc, rob = make_handles(case, K, T, num_iters=2, overlay=opt.overlay)
    engines = [exact]
    try:
        exact.setReductionMode(m.MPPI_REDUCTION_REFERENCE_ORDER)
        engines.append(make_handles(case, K, T, num_iters=2, overlay=opt.overlay)[1])
        if streams:
            engines.append(make_handles(case, K, T, num_iters=2, overlay=opt.overlay, env=dict(MPPI_AMD_NO_STREAM_MERGE="1"))[1])
        opt.apply(exact, orc)
        for e in engines[1:]:
            opt.apply(e)
        _compute(case, opt, cfg, engines, orc, rob, philox, 2)
        check_form(case, exact, tag + " [reference-order]")
        check_form(case, engines[1], tag + " [fused]", streamed=streams)
        du = check_against_oracle(case, exact, orc, tag + " [reference-order]", samples_exact=True)
        assert du <= U_TOL, "%s [reference-order]: control differs from the oracle by %g" % (tag, du)
        st, ost = exact.getStats(), orc.stats()
        names = (["nominal_sys", "real_sys"] if ctl == "robust" else ["real_sys", "nominal_sys"])[:exact.num_systems]
        for z, name in enumerate(names):
            assert getattr(st, name).baseline == ost["baseline"][z], "%s [reference-order]: %s baseline %r, oracle %r" % (
                tag, name, getattr(st, name).baseline, ost["baseline"][z])
        drift = check_against_oracle(case, engines[1], orc, tag + " [fused]", costs_exact=False)
        bound = FUSED_DRIFT.get((case["id"], set_name, (K, T)), U_TOL)
        print("FIGURE %s [fused]: control differs from the oracle by %.3e (bound %.3e)" % (tag, drift, bound))
        assert drift <= bound, "%s [fused]: control differs from the oracle by %g (bound %g; the reference-order handle is exact)" % (
            tag, drift, bound)
        if streams:
            check_form(case, engines[2], tag + " [fused, two-launch]")
            for what in ("getSampledCostSeq", "getOptimalControlSeq", "getControlSeq", "getSampledControls"):
                assert bits_equal(getattr(engines[1], what)(), getattr(engines[2], what)()), \
                    "%s: %s of the streamed handle differs from the two-launch twin" % (tag, what)
    finally:
        for e in engines:
            e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_sampler_options(gpu, case):
    for set_name in SETS:
        for K, T in KT_INJECTED:
            _run_one_iteration(case, set_name, K, T, philox=False)
        _run_one_iteration(case, set_name, *KT_PHILOX, philox=True)
        for K, T in KT_TWO_ITERS:
            _run_two_iterations(case, set_name, K, T, philox=False)
        if case["streams"]:
            _run_two_iterations(case, set_name, *KT_STREAMED, philox=True)


@pytest.mark.gpu
def test_colored_handle_refuses_independent_noise(gpu):
    """the colored-noise sampler has one distribution: MPPI_ERR_UNSUPPORTED, and the handle goes on with shared noise"""
    case = next(c for c in CASES if c["controller"] == "colored")
    opt = Options(case["model"], "colored", "table", 65, 3)
    cfg, eng, orc, _ = make_handles(case, 65, 3, overlay=opt.overlay)
    try:
        with pytest.raises(m.MPPIError) as e:
            eng.setIndependentNoise(True)
        assert e.value.status == m.MPPI_ERR_UNSUPPORTED, e.value.status
        opt.apply(eng, orc)
        _compute(case, opt, cfg, [eng], orc, None, False, 1)
        assert check_against_oracle(case, eng, orc, case["id"] + " after the refusal", samples_exact=True) <= U_TOL
    finally:
        eng.close()
