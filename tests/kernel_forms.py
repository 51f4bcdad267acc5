"""What the kernel-form test files share: the enumeration of every registered rollout kernel instantiation, the construction
of an engine handle with its oracle, one controller call on both, and the checks that follow it.

The cases come from mppi_list_models + mppi_describe_model, not from a hand-written list: one case per reachable
(registration, controller, requested kernel form).  registrations() and build_cases() ask the registry afresh on every call
(plugins register models in the middle of a session); a test module that parametrises over the cases keeps its own list, taken
when it is imported.  The float64 restatements the same files use are in tests/restate64.py.
"""
import contextlib
import os

import numpy as np

import mppi_generic_amd as m
from common import (autorally_cfg, bicycle_lstm_cfg, cartpole_cfg_lr, di_cfg, make_engine, make_oracle, make_pair, racer_cfg,
                    robust_cfg, ulp_diff)
from racer_cfgs import elevation_cfg, steering_cfg, suspension_cfg, uncertainty_cfg


@contextlib.contextmanager
def env_override(**variables):
    """sets environment variables for the block (None: unset) and puts back what was there before.  Most MPPI_AMD_* variables
    are read at mppi_create: the block decides which handles see them"""
    old = {k: os.environ.get(k) for k in variables}

    def put(values):
        for k, v in values.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    put(variables)
    try:
        yield
    finally:
        put(old)


# the edge shapes (K, T) tests/test_kernel_matrix.py and tests/test_nln_sampler.py run every case at: one rollout, partial waves
# and blocks, a ragged K >= 1000, horizons shorter than a sampler trip or a pair of steps
KT = [(1, 1), (63, 2), (65, 3), (200, 5), (1049, 9)]


# ------------------------------------------------------------------ cases -----------------------------------------------
def _plain(mk, **kw):
    def build(K, T, D):
        cfg = mk(K=K, T=T, **kw)
        cfg["D"] = D
        return cfg
    return build


# configuration builder per registered model name: (K, T, systems) -> the cfg dict of common.py
BUILDERS = {
    "cartpole": _plain(cartpole_cfg_lr),
    "double_integrator": lambda K, T, D: di_cfg(K=K, T=T, tube=D == 2),
    "double_integrator_robust": lambda K, T, D: robust_cfg(K=K, T=T, tube=D == 2),
    "racer_dubins": _plain(racer_cfg),
    "autorally_nn": _plain(autorally_cfg),
    "bicycle_slip_lstm": _plain(bicycle_lstm_cfg),
    "racer_dubins_elevation": lambda K, T, D: elevation_cfg(K=K, T=T, D=D),
    "racer_dubins_elevation_lstm_steering": lambda K, T, D: steering_cfg(K=K, T=T, D=D),
    "racer_dubins_elevation_lstm_unc": lambda K, T, D: uncertainty_cfg(K=K, T=T, D=D),
    "racer_dubins_elevation_suspension": lambda K, T, D: suspension_cfg(K=K, T=T, D=D),
}


def registrations():
    out = []
    for name in m.list_models():
        for sampler in (m.MPPI_SAMPLER_GAUSSIAN, m.MPPI_SAMPLER_COLORED):
            d = m.describe_model(name, sampler)
            if d is not None:
                out.append((name, sampler, d))
    return out


def pipeline_family(d, shape):
    """the role-pipelined kernel mppi_create runs for a shape (mppi_create's pipe_ok), or None"""
    bx, by, bz = shape
    if shape in d["replicated_lane_shapes"]:
        return "pipeline_rep" if (bx == 64 and bz == 1) else None
    if d["pipeline_fold"] and shape == (32, 1, 2):
        return "pipeline_fold"
    if d["pipeline"] and bx == 64 and by == 1:
        return "pipeline"
    return None


def make_case(reg, controller, form, kw, expect, hbm=False, refuse=None):
    name, sampler, _ = reg
    tag = "%s%s-%s-%s%s" % (name, "[colored]" if sampler else "", controller, form, "-hbm" if hbm else "")
    return dict(id=tag, model=name, controller=controller, kw=kw, expect=expect, hbm=hbm, refuse=refuse)


def build_cases():
    cases = []
    for reg in registrations():
        name, sampler, d = reg
        fused_family = lambda s: "fused_rep" if s in d["replicated_lane_shapes"] else "fused"
        controllers = ["colored"] if sampler == m.MPPI_SAMPLER_COLORED else ["vanilla", "tube"] + (["robust"] if d["rmppi"] else [])
        for ctl in controllers:
            bz = 2 if ctl == "tube" else 1
            shapes = [s for s in d["shapes"] if s[2] == bz] if ctl != "robust" else []
            for s in shapes:
                kw = dict(block_x=s[0], block_y=s[1])
                cases.append(make_case(reg, ctl, "fused%dx%dx%d" % s, dict(kw, kernel_variant=m.MPPI_KERNEL_FUSED),
                                       dict(family=fused_family(s), block=s, rows_in_hbm=False)))
                pf = pipeline_family(d, s)
                if pf:
                    cases.append(make_case(reg, ctl, "pipeline%dx%dx%d" % s, dict(kw, kernel_variant=m.MPPI_KERNEL_PIPELINE),
                                           dict(family=pf, block=s, rows_in_hbm=False)))
            if ctl == "tube" and d["pipeline_fold"]:
                # no shape requested: mppi_create folds the two systems into the lanes of a wave
                cases.append(make_case(reg, ctl, "auto-fold", dict(kernel_variant=m.MPPI_KERNEL_AUTO),
                                       dict(family="pipeline_fold", block=(32, 1, 2), rows_in_hbm=False)))
            if ctl != "robust" and shapes and d["rows_in_hbm"]:
                # MPPI_AMD_ROWS_IN_HBM=1: the sample rows in HBM at any horizon, on the first registered shape of each kind
                first = shapes[0]
                cases.append(make_case(reg, ctl, "fused%dx%dx%d" % first,
                                       dict(block_x=first[0], block_y=first[1], kernel_variant=m.MPPI_KERNEL_FUSED),
                                       dict(family=fused_family(first), block=first, rows_in_hbm=True), hbm=True))
                piped = [s for s in shapes if pipeline_family(d, s)]
                if piped:
                    s = piped[0]
                    cases.append(make_case(reg, ctl, "pipeline%dx%dx%d" % s,
                                           dict(block_x=s[0], block_y=s[1], kernel_variant=m.MPPI_KERNEL_PIPELINE),
                                           dict(family=pipeline_family(d, s), block=s, rows_in_hbm=True), hbm=True))
            if ctl == "robust":
                for bx in (64, 32):
                    cases.append(make_case(reg, ctl, "fused%dx1x2" % bx, dict(block_x=bx, kernel_variant=m.MPPI_KERNEL_FUSED),
                                           dict(family="rmppi", block=(bx, 1, 2), rows_in_hbm=False)))
                if d["rmppi_pipeline"]:
                    # the role-pipelined Robust kernel keeps its sample rows in HBM by design (the rings take the LDS)
                    cases.append(make_case(reg, ctl, "pipeline64x1x2", dict(kernel_variant=m.MPPI_KERNEL_PIPELINE),
                                           dict(family="rmppi_pipeline", block=(64, 1, 2), rows_in_hbm=True)))
                else:
                    cases.append(make_case(reg, ctl, "pipeline-refused", dict(kernel_variant=m.MPPI_KERNEL_PIPELINE), None,
                                           refuse=m.MPPI_ERR_LAUNCH_SHAPE))
                cases.append(make_case(reg, ctl, "16x1x2-refused", dict(block_x=16, kernel_variant=m.MPPI_KERNEL_FUSED), None,
                                       refuse=m.MPPI_ERR_LAUNCH_SHAPE))
            # a pipeline request on a shape that has no pipelined form is refused, never run as something else
            unpiped = [s for s in shapes if not pipeline_family(d, s)]
            if unpiped:
                s = unpiped[0]
                cases.append(make_case(reg, ctl, "pipeline%dx%dx%d-refused" % s,
                                       dict(block_x=s[0], block_y=s[1], kernel_variant=m.MPPI_KERNEL_PIPELINE), None,
                                       refuse=m.MPPI_ERR_LAUNCH_SHAPE))
    return cases


def expects_streamed_merge(case, d, K, T, C, philox, reduction_fused=True):
    """streamMergeApplies() (engine_iteration.hip) for this case's handle: the one-system role pipeline at 64x1x1 with its
    sample rows in LDS, in-kernel Philox noise, the fused reduction, no Tsallis weights (no case sets them), not Robust,
    T*C % 4 == 0, at most 256 blocks, and a model that supports it"""
    e = case["expect"]
    return bool(philox and reduction_fused and e["family"] == "pipeline" and e["block"] == (64, 1, 1) and not e["rows_in_hbm"]
                and case["controller"] in ("vanilla", "colored") and (T * C) % 4 == 0 and -(-K // 64) <= 256
                and d["streamed_merge"])


# tests/test_kernel_sequence.py (and, for its Philox shape, tests/test_sharded_matrix.py): fused (default) handles whose
# control drifts past U_TOL from the oracle within the 3 calls, while the reference-order
# handle of the same sequence stays within it: the fused merge sums the weighted samples in another order than the
# reference, each iteration starts from the previous one's u*, and the difference grows over 9 iterations through the RACER
# dynamics (the Tube nominal control, which is re-optimised from its own smoothed past, most of all).  Every other check of
# these handles — path, launch counts, float64 softmin / statistics / smoothing, trajectories — holds unchanged.
# (case id, sequence) -> bound: the largest control / nominal control difference measured over the 3 calls, rounded up.
FUSED_DRIFT = {
    ("racer_dubins-tube-fused16x1x2", "injected"): 1.3e-5,                         # measured 1.283e-5
    ("racer_dubins-tube-auto-fold", "injected"): 1.35e-5,                          # measured 1.313e-5
    ("racer_dubins_elevation_lstm_steering-robust-fused32x1x2", "philox"): 1.15e-5,  # measured 1.109e-5
    ("racer_dubins_elevation_lstm_unc-tube-fused64x1x2", "injected"): 1.3e-5,      # measured 1.252e-5
    ("racer_dubins_elevation_suspension-tube-fused64x4x2", "philox"): 1.05e-5,     # measured 1.031e-5
    ("racer_dubins_elevation_suspension-tube-fused64x1x2", "philox"): 1.05e-5,     # measured 1.031e-5
    ("racer_dubins_elevation_suspension-tube-fused64x4x2-hbm", "philox"): 1.05e-5,  # measured 1.031e-5
    ("racer_dubins_elevation_suspension-tube-fused64x4x2", "injected"): 1.4e-5,    # measured 1.360e-5
    ("racer_dubins_elevation_suspension-tube-fused64x1x2", "injected"): 1.4e-5,    # measured 1.360e-5
    ("racer_dubins_elevation_suspension-tube-fused64x4x2-hbm", "injected"): 1.4e-5,  # measured 1.360e-5
}


# ------------------------------------------------------------------ handles ---------------------------------------------
def _colored_params(C):
    return ([1.0, 0.5][:C], 0.97, 0.0)


def make_handles(case, K, T, num_iters=1, overlay=None, sampler=None, env=None):
    """(cfg, engine, oracle, RobustOracle or None) of a case at (K, T), the engine with save_samples.
    A case that carries its own builder (case["build"]) is configured by it alone; the cases of build_cases() take BUILDERS, the
    colored-noise parameters, and for Robust MPPI the coefficients [0.2, 0.1].
    overlay: cfg entries that replace all of that — the sampler options of tests/test_sampler_options_matrix.py.
    sampler: an MPPI_SAMPLER_* constant; None is the controller's own.
    env: environment variables mppi_create is to see, beside the case's own MPPI_AMD_ROWS_IN_HBM (cases with an "hbm" entry)"""
    ctl = case["controller"]
    D = 2 if ctl in ("tube", "robust") else 1
    own = "build" in case
    cfg = (case["build"] if own else BUILDERS[case["model"]])(K, T, D)
    cfg["D"] = D
    cfg["num_iters"] = num_iters
    if ctl == "colored":
        cfg["colored"] = _colored_params(len(cfg["control_cost_coeff"]))
    if ctl == "robust" and not own:
        cfg["control_cost_coeff"] = [0.2, 0.1][:len(cfg["control_cost_coeff"])]
    cfg.update(overlay or {})
    kw = dict(case["kw"], save_samples=True)
    if sampler is not None:
        kw["sampler"] = sampler
    env = dict(env or {})
    if "hbm" in case:
        env["MPPI_AMD_ROWS_IN_HBM"] = "1" if case["hbm"] else "0"
    with env_override(**env):
        if ctl == "robust":
            # 9 x 32 candidate rollouts as bench.py; fewer rollouts than that take the smallest candidate set (3, odd) that fits
            nc, ns = (9, 32) if K >= 9 * 32 else (3, K // 3)
            eng, orc, rob = make_pair(cfg, nc=nc, ns=ns, **kw)
        else:
            eng, orc, rob = make_engine(cfg, tube=D == 2, **kw), make_oracle(cfg), None
    return cfg, eng, orc, rob


# ------------------------------------------------------------------ one call --------------------------------------------
def compute_once(case, engines, orc, rob, cfg, stride, noise, philox, seed, candidate_noise=None, first_cycle=True,
                 seed_before_first_cycle=True):
    """one computeControl(cfg["x0"], stride) of every engine and the matching call of the oracle (rob for Robust MPPI).
    noise: what the oracle is handed, one slab per iteration — and, unless philox, what the engines are injected with.
    philox: the engines draw in-kernel noise after setSeed(seed); seed None leaves the generator as the caller has set it.
    Robust MPPI: updateImportanceSamplingControl comes first, the oracle's with candidate_noise; on the first cycle (no
    nominal state yet, no candidates, no noise drawn: robust_mppi_controller.cu:508-633) candidate_noise is None and the
    feedback gains are set after it.  seed_before_first_cycle=False moves setSeed behind the first cycle, where
    tests/test_kernel_matrix.py has always had it."""
    ctl = case["controller"]
    x0 = cfg["x0"]

    def set_seed():
        if philox and seed is not None:
            for e in engines:
                e.setSeed(seed)

    if ctl != "robust" or seed_before_first_cycle:
        set_seed()
    if not philox:
        for e in engines:
            e.injectNoise(noise)
    if ctl == "robust":
        for e in engines:
            e.updateImportanceSamplingControl(x0, stride)
            if first_cycle:
                e.setFeedbackGains(robust_gains(cfg["T"], e.STATE_DIM, e.CONTROL_DIM))
        rob.update_importance_sampling(x0, stride, candidate_noise)
        if first_cycle:
            rob.set_gains(robust_gains(cfg["T"], engines[0].STATE_DIM, engines[0].CONTROL_DIM))
        if not seed_before_first_cycle:
            set_seed()
    for e in engines:
        e.computeControl(x0, stride)
    if ctl == "colored":
        orc.colored_compute_control(x0, stride, noise, *cfg["colored"])
    elif ctl == "robust":
        rob.compute_control(x0, stride, noise)
    elif ctl == "tube":
        orc.tube_compute_control(x0, stride, noise)
    else:
        orc.vanilla_compute_control(x0, stride, noise)


def robust_gains(T, S, C):
    """the feedback gains every Robust case runs with"""
    return np.random.default_rng(5).uniform(-0.3, 0.3, (T, S, C)).astype(np.float32)


# ------------------------------------------------------------------ checks ----------------------------------------------
def check_form(case, eng, tag, streamed=False):
    info = eng.getLaunchInfo()
    got = {k: info[k] for k in ("family", "block", "rows_in_hbm")}
    assert got == case["expect"], "%s: launched %s, the case expects %s" % (tag, got, case["expect"])
    assert info["streamed_merge"] == streamed, "%s: streamed_merge %s, expected %s" % (tag, info["streamed_merge"], streamed)


def check_against_oracle(case, eng, orc, tag, costs_exact=True, samples_exact=False, show=False):
    """costs (and dumped samples) 0 ulp where the handle reduces as the oracle does -> the largest difference of u* and, for
    Tube and Robust MPPI, of the nominal u* from the oracle's; the caller asserts its own bound on that.
    show: print the cost and u* figures before anything is asserted"""
    costs = eng.getSampledCostSeq()
    assert np.isfinite(costs).all(), tag
    du = float(np.abs(eng.getControlSeq() - orc.control()).max())
    if show:
        print("%s: costs %d ulp" % (tag, int(ulp_diff(costs, orc.costs()).max())))
        print("%s: u* %g" % (tag, du))
    if costs_exact:
        dc = int(ulp_diff(costs, orc.costs()).max())
        assert dc == 0, "%s: sampled costs differ from the oracle by up to %d ulp" % (tag, dc)
    if samples_exact:
        dv = int(ulp_diff(eng.getSampledControls(), orc.samples()).max())
        assert dv == 0, "%s: dumped samples differ from the oracle's clamped samples by up to %d ulp" % (tag, dv)
    if case["controller"] in ("tube", "robust"):
        du = max(du, float(np.abs(eng.getNominalControlSeq() - orc.nominal_control()).max()))
    return du
