"""Scenario builders and the +inf-aware float64 restatement for tests/test_softmin_edges.py: the softmin reduction at infinite,
tied and far-apart costs.

Every scenario runs on the two double-integrator models only: plain arithmetic, no table look-up, no value-dependent loop, so
a non-finite value cannot become an address.  A scenario is a configuration overlay (cost parameters, lambda, x0) and the
noise of one computeControl call; what the costs then ARE is read off the oracle (tests/test_softmin_edges.py asserts the
design on the CPU before a kernel sees it), never assumed from the noise: the sample rule exempts rollout 0 from the noise.

How a rollout is driven to +inf, per model:
  double_integrator         DoubleIntegratorCircleCost adds crash_cost off the annulus and nothing on it: crash_cost = +inf and
                            a noise row whose first channel is the constant 200 (off the annulus within a few steps);
  double_integrator_robust  DoubleIntegratorRobustCost ramps linearly up to crash_cost ON the track (linInterp), so an infinite
                            crash_cost costs every rollout +inf or NaN (0 * inf on the centre line) and cannot be the lever.
                            There the crash rows carry 1e21 in the first channel: the squared speed error overflows fp32 within
                            two steps, and the cost is +inf by arithmetic alone (crash_cost stays finite).  all_inf and overflow
                            work on this model as on the other (off the track the cost adds crash_cost itself).
Colored cases take a spectrum: the real DC coefficient of channel 0 plays the constant row's part (it gives a first channel
growing linearly with t).
"""
import functools

import numpy as np

import mppi_generic_amd as m
import pyoracle as po
from common import PHILOX_SEED, host_noise, host_spectrum
from kernel_forms import make_handles
from restate64 import EPS32, SOFTMIN_RTOL

MODELS = ("double_integrator", "double_integrator_robust")
INJECTED_KT = (200, 9)       # as tests/test_kernel_sequence.py
PHILOX_KT = (1049, 12)
RECORD_EDGE_KT = [(4096, 5), (4112, 5)]  # 256 and 257 records of 16 rollouts: combineWave's last one-pass / first two-pass count
INJECTED = ("mixed_inf", "one_finite", "all_inf", "tied_min", "all_tied", "far_zero", "far_subnormal", "overflow")
PHILOX = ("philox_mixed", "philox_all_inf")
NON_FINITE = ("mixed_inf", "one_finite", "all_inf", "overflow", "philox_mixed", "philox_all_inf")  # some cost is +inf
ALL_INF = ("all_inf", "philox_all_inf")
ZERO_WEIGHT_RERUN = ("mixed_inf", "far_zero", "overflow")  # re-run with the crash rows' second channel * 1e3
BASE_SCALE = np.float32(0.05)  # base rows: host noise scaled down, they stay on the annulus
OFF_TRACK_X0 = np.array([3.0, 0.0, 0.0, 1.0], np.float32)
FAR_BLOCK = slice(64, 128)     # the all-crash 64-rollout block (and the 32- and 16-rollout blocks inside it)
PHILOX_ITERS = 2               # the in-kernel merge of the streamed path happens in the second launch


def crash_rows(K):
    """all of rollouts 64..127, every third rollout of 0..63 (1, 4, ..: rollout 0 takes no noise) and rollout K - 1"""
    return np.array(sorted(set(range(64, min(128, K))) | set(range(1, min(64, K), 3)) | {K - 1}))


def _cost(crash_cost):
    c = m.DoubleIntegratorCircleCostParams()
    c.crash_cost = crash_cost
    return c


def _crash_value(model, colored, finite):
    """the constant a crash row carries in its first channel (injected rows) or in its real DC coefficient (spectrum)"""
    big = 200.0 if (finite or model == "double_integrator") else 1e21
    return big * 100.0 if colored else big


def _set_rows(noise, rows, value, colored):
    if colored:
        noise[0, rows, 0, 0, 0] = value   # z [iters][K][C][T+1][2]
    else:
        noise[0, rows, :, 0] = value      # eps [iters][K][T][C]


def scale_second_channel(noise, rows, colored, factor=1e3):
    out = noise.copy()
    if colored:
        out[0, rows, 1] *= np.float32(factor)
    else:
        out[0, rows, :, 1] *= np.float32(factor)
    return out


def _base(K, T, colored):
    gen = host_spectrum if colored else host_noise
    return gen(1, K, T, 2, seed=K + T) * BASE_SCALE


def oracle_costs(case, K, T, overlay, noise, philox=False, num_iters=1):
    """the oracle's costs [D][K] of the LAST iteration and its statistics for one call of a case (no engine involved: the
    engine half of make_handles needs a device, so the oracle is built by itself here)"""
    from kernel_forms import BUILDERS, robust_gains
    from common import make_oracle
    ctl = case["controller"]
    D = 2 if ctl in ("tube", "robust") else 1
    cfg = BUILDERS[case["model"]](K, T, D)
    cfg["D"], cfg["num_iters"] = D, num_iters
    if ctl == "colored":
        cfg["colored"] = ([1.0, 0.5], 0.97, 0.0)
    if ctl == "robust":
        cfg["control_cost_coeff"] = [0.2, 0.1]
    cfg.update(overlay)
    orc = make_oracle(cfg)
    if ctl == "colored":
        orc.colored_compute_control(cfg["x0"], 1, noise, *cfg["colored"])
    elif ctl == "robust":
        nc, ns = (9, 32) if K >= 9 * 32 else (3, K // 3)
        rob = po.RobustOracle(orc, 1000.0, nc, ns)
        rob.update_importance_sampling(cfg["x0"], 1, None)
        rob.set_gains(robust_gains(T, orc.S, orc.C))
        rob.compute_control(cfg["x0"], 1, noise)
    elif ctl == "tube":
        orc.tube_compute_control(cfg["x0"], 1, noise)
    else:
        orc.vanilla_compute_control(cfg["x0"], 1, noise)
    return orc.costs().copy()


def _key(case):
    return (case["model"], case["controller"])


_CASE_OF_KEY = {}


@functools.lru_cache(maxsize=None)
def _scenario(name, key, K, T):
    case = _CASE_OF_KEY[key]
    model, ctl = key
    colored = ctl == "colored"
    if name in PHILOX:
        # in-kernel Philox noise: the oracle is handed po.philox_normal / po.philox_spectrum of generation 0, 1
        gen = (lambda g: po.philox_spectrum(PHILOX_SEED, g, K, T, 2)) if colored else (lambda g: po.philox_normal(PHILOX_SEED, g, K, T, 2))
        noise = np.stack([gen(g) for g in range(PHILOX_ITERS)])
        if name == "philox_all_inf":
            overlay = dict(cost=_cost(np.inf), x0=OFF_TRACK_X0.copy())
        else:
            # std_dev (PHILOX_STD_DEV) chosen so that within T = 12 steps roughly half of the rollouts end at +inf (asserted on
            # the CPU, both iterations).  The robust cost cannot take an infinite crash_cost (module docstring): 3e38 there, and the running
            # sum of two crash steps is +inf
            overlay = dict(cost=_cost(np.inf if model == "double_integrator" else 3e38), std_dev=[PHILOX_STD_DEV[(model, colored)]] * 2)
        return dict(name=name, overlay=overlay, noise=noise, philox=True, num_iters=PHILOX_ITERS, rows=None, colored=colored)
    noise = _base(K, T, colored)
    rows = crash_rows(K)
    overlay = {}
    finite_crash = name in ("far_zero", "far_subnormal", "overflow")
    big = _crash_value(model, colored, finite_crash)
    if name in ("mixed_inf", "far_zero", "far_subnormal", "overflow"):
        _set_rows(noise, rows, big, colored)
    elif name == "one_finite":
        rows = np.arange(K)
        _set_rows(noise, rows, big, colored)
    elif name == "all_inf":
        rows = np.arange(0)
        overlay["x0"] = OFF_TRACK_X0.copy()
    elif name == "tied_min":
        base_costs = oracle_costs(case, K, T, {}, noise)[-1]
        best = 1 + int(np.argmin(base_costs[1:]))  # (rollout 0 has no noise row to copy)
        rows = np.array([k for k in (10, 70, 130, K - 10) if k != best])
        noise[0, rows] = noise[0, best]
    elif name == "all_tied":
        rows = np.arange(K)
        noise[0, :] = noise[0, 1]
    if name in ("mixed_inf", "one_finite", "all_inf"):
        overlay["cost"] = _cost(np.inf if (model == "double_integrator" or name == "all_inf") else 100.0)
    elif name in ("far_zero", "far_subnormal"):
        overlay["cost"] = _cost(1000.0)
        overlay["lambda_"] = 2.0
        if name == "far_subnormal":
            c = oracle_costs(case, K, T, overlay, noise)
            z = c.shape[0] - 1  # the system the handle's u* follows (Robust: the real one); asserted for every system on the CPU
            overlay["lambda_"] = float(np.float32((float(c[z, FAR_BLOCK].min()) - float(c[z].min())) / 95.0))
    elif name == "overflow":
        overlay["cost"] = _cost(3e38)
    return dict(name=name, overlay=overlay, noise=noise, philox=False, num_iters=1, rows=rows, colored=colored)


# (model, colored) -> std_dev of both channels; +inf share measured on the oracle: 0.48 / 0.55 and 0.55 / 0.59 in iteration 1
PHILOX_STD_DEV = {("double_integrator", False): 30.0, ("double_integrator", True): 12.0,
                  ("double_integrator_robust", False): 6.0, ("double_integrator_robust", True): 4.0}


def scenario(name, case, K, T):
    """dict(overlay: cfg entries for make_handles, noise: what the oracle is handed (and the engine, unless philox), philox,
    num_iters, rows: the rollouts whose noise rows the scenario rewrote, colored).  Built once per (scenario, model,
    controller, K, T) and shared: callers must not modify it"""
    _CASE_OF_KEY.setdefault(_key(case), dict(model=case["model"], controller=case["controller"]))
    return _scenario(name, _key(case), K, T)


def scenario_handles(case, sc, K, T, env=None):
    return make_handles(case, K, T, num_iters=sc["num_iters"], overlay=dict(sc["overlay"]), env=env)


def scale_arg32(rho_b, rho, lambda_):
    """(rho_b - rho) / lambda as the engine forms it: fl(fl(rho_b - rho) * fl(1 / lambda)) with lambda rounded to fp32"""
    lam32 = np.float32(lambda_)
    lambda_inv = np.float32(1.0 / np.float64(lam32))
    return float(np.float32(np.float32(rho_b) - np.float32(rho)) * lambda_inv)


# ------------------------------------------------------------------ float64, +inf aware --------------------------------
def softmin64_inf(costs, v, lambda_):
    """restate64.softmin64 with the rule for +inf: such a rollout has weight 0 (exp(-inf)), whatever its samples; the baseline is
    the minimum over ALL costs, and when that is +inf nothing has weight: NaN"""
    c = np.asarray(costs, np.float64)
    v = np.asarray(v, np.float64)
    b = c.min()
    if not np.isfinite(b):
        return np.full(v.shape[1:], np.nan)
    fin = np.isfinite(c)
    w = np.zeros_like(c)
    w[fin] = np.exp(-(c[fin] - b) / lambda_)
    return (w[fin, None, None] * v[fin]).sum(0) / w.sum()


def stats64_inf(costs, lambda_):
    """restate64.stats64 (core/mppi_common.cu:1065-1081 in float64, first-order fp32 bounds) with the rule for +inf: weight 0
    and relative error 0 (exp(-inf) is exactly 0 in any arithmetic), and the rollout still counts in K.  All costs +inf: the
    baseline is +inf and every other value NaN (bounds 0).  On finite costs this is stats64, value for value."""
    c = np.asarray(costs, np.float32).astype(np.float64)
    K = c.size
    u = EPS32 / 2
    b = c.min()
    keys = ("baseline", "normalizer", "free_energy_mean", "free_energy_variance", "free_energy_modified_variance")
    if not np.isfinite(b):
        return dict(zip(keys, (b,) + (np.nan,) * 4)), dict.fromkeys(keys, 0.0)
    fin = np.isfinite(c)
    x = np.zeros_like(c)
    x[fin] = (c[fin] - b) / lambda_
    w = np.where(fin, np.exp(-x), 0.0)
    d = np.where(fin, 3 * u * x + 4 * u, 0.0)
    e1 = (w * d).sum() / w.sum() + K * u
    e2 = (w * w * (2 * d + u)).sum() / (w * w).sum() + K * u
    mean, mean2 = w.mean(), (w * w).mean()
    fe = -lambda_ * np.log(mean) + b
    var = lambda_ * (mean2 - mean * mean)
    q = var / (mean * np.sqrt(K))
    mod = lambda_ * (q + 0.5 * q * q)
    d_fe = lambda_ * e1 + 8 * u * (lambda_ * abs(np.log(mean)) + abs(b))
    d_var = lambda_ * (e2 * mean2 + (2 * e1 + u) * mean * mean) + 3 * u * abs(var)
    d_q = d_var / (mean * np.sqrt(K)) + abs(q) * (e1 + 6 * u)
    d_mod = lambda_ * (1 + abs(q)) * d_q + 4 * u * abs(mod)
    vals = dict(zip(keys, (b, w.sum(), fe, var, mod)))
    bounds = dict(zip(keys, (0.0, SOFTMIN_RTOL * w.sum(), d_fe, d_var, d_mod)))
    return vals, bounds


# ------------------------------------------------------------------ written records, edge sets -------------------------
# beside tests/test_sharded_matrix.py's MERGE_SETS (which stay as they are): records with rho = +inf, U = eta = eta2 = 0 — what
# the rollout epilogue writes for a block whose rollouts all cost +inf — at the first, a middle and the last position, several
# of them, all of them; and records whose scale factor exp(-(rho_b - rho) / lambda) lies below the smallest normal fp32 number
EDGE_MERGE_SETS = ("inf_first", "inf_middle", "inf_last", "inf_several", "inf_all", "subnormal_band")
SUBNORMAL_FLOOR = 2.0 ** -126  # see merge_reference_floor


def edge_merge_records(kind, W, D, TC, lam, seed):
    from test_sharded_matrix import merge_records
    rec = merge_records("random", W, D, TC, lam, seed)
    if kind == "subnormal_band":
        # every record but the first 88.5 .. 102.5 lambda above it
        rng = np.random.default_rng(seed + 1)
        rec[1:, :, TC] = rec[0, :, TC][None] + np.float32(lam) * rng.uniform(88.5, 102.5, (W - 1, D)).astype(np.float32)
        return rec
    # (inf_several leaves record 1 finite in every world, 2 and 3 included)
    where = {"inf_first": [0], "inf_middle": [W // 2], "inf_last": [W - 1], "inf_several": sorted({0, W // 2, W - 1} - {1}),
             "inf_all": list(range(W))}[kind]
    for b in where:
        rec[b] = 0.0
        rec[b, :, TC] = np.inf
    return rec
