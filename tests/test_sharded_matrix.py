"""Every registered kernel form with K split over ranks, held to the UN-sharded oracle rank by rank.

tests/test_kernel_matrix.py and tests/test_kernel_sequence.py hold a single handle of every registered (model, sampler,
controller, kernel form) to the oracle.  A handle created with rank= / world_size= owns rollouts [rank K/world,
(rank + 1) K/world) of the same problem: the sampler must then use the GLOBAL rollout index for the "rollout 0 takes the mean"
rule, for the pure-noise tail and for the Philox counter, and every kernel family reaches the sampler through other lines.  A
form that used the local index would be wrong on ranks > 0 only, in one to sixteen rollouts of K — far below what a
comparison of u* can see.  So this file compares what each rank itself computed.

Part A  every non-Robust runnable case of test_kernel_matrix.build_cases() (the same enumeration, not a second list), all
        ranks as handles of one process, the exchange driven by the caller and staged through the host:
          every rank: uploadState, iterationLocal, readSendRecord -> concatenate -> every rank: writeRecvRecords, iterationMerge.
        Nothing in that path waits on another stream, so eight ranks run on any number of hardware queues.
        Shapes (K, world, T), injected noise, one iteration: (8, 8, 2) one rollout per rank; (126, 2, 3) a partial wave;
        (1047, 3, 9) five blocks + 29 per rank in an odd world; colored cases also the radix-4 edges (195, 3, 16) and
        (130, 2, 17).  Rank r gets rows [r K/world, (r + 1) K/world) of the noise the oracle gets whole.  In-kernel Philox:
        (1600, 8, 12), three iterations by hand after setSeed, the oracle handed generation 0, 1, 2 over the whole K (the
        generation advances by one per rollout launch, see test_kernel_sequence.py).  T*C is a multiple of 4 there and ragged
        in the injected shapes: both load paths of the gathered merge run.
        Per iteration: the launched family / block / rows-in-HBM of every rank; every rank's costs and clamped samples 0 ulp
        from the oracle's slice (the oracle rolls out from the engine's OWN current mean, identical on all ranks, so the bar
        stays at 0 ulp although the fused merge rounds differently from the oracle's); u* of every rank within 1e-5 of the
        oracle's un-sharded, chained iterate; u* and statistics of every rank bit-identical to rank 0's; and in float64, sharing
        no code with engine or oracle, u* against the softmin of the concatenated dumps and the statistics within stats64's
        bounds at the global K — per system for Tube.
        With pure_noise_trajectories_percentage = 0.01 the pure-noise tail lies in the last rank only (K = 8 has none) and the
        mean rollout in rank 0 only, at every shape here (asserted below from the reference's own formula): a local-index
        mistake shows on every other rank.
        Robust MPPI is left out on purpose: its sharded computeControl shares the candidate evaluation over the P2P mailbox or
        RCCL, which the caller-driven exchange does not offer; tests/test_rmppi.py keeps that path.

Part B  the gathered-layout merge (combineKernel over [world][D][T*C + 4] records with world-major strides) on records the
        test writes itself: world 2, 3, 8, 16; one and two systems; T*C = 4, 9, 200, 201 (the quad-load path, the scalar path,
        more than one column wave each way); random records, all baselines equal, one dominant rank first / last with every
        other scale factor exactly 0.  Reference: common.merge_records_numpy in float64, with first-order rounding bounds
        computed from the inputs (see _merge_reference).  In the dominant sets the U of every underflowed record is then
        replaced by 1e30: not one bit of u* or of the statistics may change.

Part C  CPU: the case list covers every registration; the float64 merge rule equals the softmin of the concatenation; the
        special-trajectory placement; the inputs of part B stay out of the range where the fp32 scale factor is subnormal;
        refusals the suite did not assert yet.
"""
import numpy as np
import pytest

import mppi_generic_amd as m
import pyoracle as po
from common import (PHILOX_SEED, U_TOL, cartpole_cfg, colored_cartpole, di_cfg, host_noise, host_spectrum, make_engine,
                    merge_records_numpy, ulp_diff)
from kernel_forms import BUILDERS, FUSED_DRIFT, build_cases, make_handles, registrations
from restate64 import EPS32, SOFTMIN_RTOL, bits_equal, softmin64, stats64, stats_of

SHAPES = [(8, 8, 2), (126, 2, 3), (1047, 3, 9)]          # (K, world, T), injected noise
SHAPES_COLORED = SHAPES + [(195, 3, 16), (130, 2, 17)]   # + the radix-4 edges of the colored-noise sampler
PHILOX_SHAPE = (1600, 8, 12)
PHILOX_ITERS = 3
PURE_PCT = 0.01  # common.make_engine / make_oracle default
UNIT = EPS32 / 2  # u = 2^-24


def sharded_cases():
    return [c for c in build_cases() if not c["refuse"] and c["controller"] != "robust"]


SHARDED_CASES = sharded_cases()


def _shapes(case):
    return SHAPES_COLORED if case["controller"] == "colored" else SHAPES


# ------------------------------------------------------------------ part C: CPU ---------------------------------------
def test_every_registration_has_a_sharded_case(lib):
    """one sharded case per non-Robust runnable case of build_cases(), and every registration that has such a case has a
    sharded one: a registration added to the registry is run sharded or fails here"""
    runnable = [c for c in build_cases() if not c["refuse"] and c["controller"] != "robust"]
    ids = [c["id"] for c in sharded_cases()]
    assert ids == [c["id"] for c in runnable] and len(ids) == len(set(ids))
    # the parametrised list was taken when this module was imported; a test that ran since may have loaded a plugin model
    # into the process-wide registry (tests/test_plugin_model.py), which has no configuration builder
    assert [c["id"] for c in SHARDED_CASES] == [c["id"] for c in runnable if c["model"] in BUILDERS]
    for name, sampler, _ in registrations():
        prefix = name + ("[colored]" if sampler else "") + "-"
        if any(c["id"].startswith(prefix) for c in runnable):
            assert any(i.startswith(prefix) for i in ids), "registration %s has no sharded case" % prefix


def _is_pure_noise(k, K, pct=PURE_PCT):
    """gaussian.cu:108 / :512: the int index compared in float against (1 - p) * K"""
    return np.float32(k) >= (np.float32(1.0) - np.float32(pct)) * np.float32(K)


def test_special_rollouts_lie_in_the_first_and_the_last_rank_only():
    """the mean rollout (global index 0) in rank 0, the pure-noise tail in the last rank and nowhere else, and no LOCAL index
    reaches the tail's threshold: a sampler that took the local index would have no pure-noise rollout at all in the last
    rank and a mean rollout in every rank"""
    for K, W, _ in SHAPES_COLORED + [PHILOX_SHAPE]:
        assert K % W == 0 and 1 < W <= 8, (K, W)
        Kl = K // W
        pure = [k for k in range(K) if _is_pure_noise(k, K)]
        # (K = 8 has no tail, 0.99 * 8 > 7: with one rollout per rank that shape is about the mean rule on ranks 1..7)
        assert bool(pure) == (K >= 100), (K, W)
        assert {k // Kl for k in pure} <= {W - 1}, (K, W, pure)
        assert not any(_is_pure_noise(k, K) for k in range(Kl)), (K, W)  # what a local index would give


@pytest.mark.parametrize("sizes,spread,dominant", [((5, 1, 64, 29), 30.0, None), ((349, 349, 349), 5.0, None),
                                                   ((1, 1, 1, 1, 1, 1, 1, 1), 3.0, None), ((63, 63), 0.0, None),
                                                   ((200, 17, 3), 4.0, 1), ((8, 8, 8), 2.0, 2)])
def test_merging_float64_shard_records_is_the_softmin_of_the_concatenation(sizes, spread, dominant):
    """common.merge_records_numpy on per-shard softmin records (U_b = sum w v, rho_b = min, eta_b = sum w, all float64) equals
    softmin64 over all rollouts: ragged shards, single-rollout shards, equal costs, and one shard that dominates (every other
    shard 300 lambda and more above it)"""
    rng = np.random.default_rng(sum(sizes))
    lam, T, C = 0.7, 5, 2
    costs = [50.0 + spread * rng.random(n) for n in sizes]
    if dominant is not None:
        costs = [c + (0.0 if b == dominant else 300 * lam * (1 + b)) for b, c in enumerate(costs)]
    vs = [rng.standard_normal((n, T, C)) for n in sizes]
    U, rho, eta = [], [], []
    for c, v in zip(costs, vs):
        w = np.exp(-(c - c.min()) / lam)
        U.append((w[:, None, None] * v).sum(0).reshape(-1))
        rho.append(c.min())
        eta.append(w.sum())
    u, rho_min, eta_tot = merge_records_numpy(np.array(U), np.array(rho), np.array(eta), lam)
    call, vall = np.concatenate(costs), np.concatenate(vs)
    want = softmin64(call, vall, lam).reshape(-1)
    assert np.abs(u - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert rho_min == call.min()
    assert abs(eta_tot - np.exp(-(call - call.min()) / lam).sum()) <= 1e-12 * eta_tot


def test_create_refuses_rollouts_not_divisible_by_the_world(lib):
    """mppi_create: num_rollouts % world_size != 0 is MPPI_ERR_INVALID_ARG (checked before a device is looked for), as is a
    rank outside the world"""
    for K, rank, world in ((1047, 0, 2), (8, 1, 3), (64, 2, 2), (64, -1, 2)):
        with pytest.raises(m.MPPIError) as e:
            m.VanillaMPPIController("cartpole", K, 5, 0.02, 1.0, rank=rank, world_size=world)
        assert e.value.status == m.MPPI_ERR_INVALID_ARG, (K, rank, world, e.value.status)


# ---- part B inputs and reference (CPU) ----
MERGE_WORLDS = (2, 3, 8, 16)
MERGE_SETS = ("random", "equal", "dominant_first", "dominant_last")
# (id, configuration, D, C, T): T*C = 4, 9, 200, 201 for one system (Cartpole, C = 1); for two systems the double integrator
# Tube (C = 2) gives the multiples of 4 and, since C = 2 cannot make an odd T*C, its ragged neighbours 10 and 202; Cartpole Tube
# gives 9 and 201 themselves
MERGE_PROBLEMS = [("cartpole-D1-TC%d" % T, "cartpole", 1, 1, T) for T in (4, 9, 200, 201)] + \
                 [("double_integrator-D2-TC%d" % (2 * T), "double_integrator", 2, 2, T) for T in (2, 5, 100, 101)] + \
                 [("cartpole-D2-TC%d" % T, "cartpole", 2, 1, T) for T in (9, 201)]
MERGE_LAMBDA = {"cartpole": 0.3, "double_integrator": 2.0}  # 0.3: lambda and 1 / lambda both round in fp32


def _merge_K(W):
    return 48 * W  # a multiple of 16; K / W = 48 rollouts behind every record


def merge_records(kind, W, D, TC, lam, seed):
    """records [W][D][TC + 4] float32 = [U | rho, eta, sum w^2, pad] (reduce_kernels.hpp) of one record set"""
    rng = np.random.default_rng(seed)
    n = _merge_K(W) // W
    rec = np.zeros((W, D, TC + 4), np.float32)
    eta = rng.uniform(1.0, n, (W, D))
    rec[:, :, :TC] = rng.standard_normal((W, D, TC)) * eta[:, :, None]
    rec[:, :, TC + 1] = eta
    # sum w^2 of n weights in (0, 1] with sum eta: between eta^2 / n and eta
    rec[:, :, TC + 2] = eta * eta / n + rng.random((W, D)) * (eta - eta * eta / n)
    base = 37.5
    if kind == "random":
        rho = base + lam * rng.uniform(0.0, 10.0, (W, D))
    elif kind == "equal":
        rho = np.full((W, D), base)
    else:
        # every record but the dominant one 210 lambda and more above it, up to 1e4 lambda
        rho = base + lam * np.exp(rng.uniform(np.log(210.0), np.log(1e4), (W, D)))
        rho[0 if kind == "dominant_first" else W - 1] = base + lam * rng.uniform(0.0, 1.0, D)
    rec[:, :, TC] = rho
    return rec


def _merge_x(rec, TC, lam32):
    """x_b = (rho_b - rho_min) / lambda [W][D] in float64 from the fp32 values the engine reads"""
    rho = rec[:, :, TC].astype(np.float64)
    return (rho - rho.min(0)) / float(lam32)


def test_merge_inputs_avoid_the_subnormal_scale_factors():
    """every (rho_b - rho_min) / lambda is <= 80 or >= 200: between those the fp32 scale factor exp(-x) is subnormal or nearly
    so (det::exp returns exactly 0 below -104, tests/test_det_math.py) and no useful rounding bound exists"""
    for _, model, D, C, T in MERGE_PROBLEMS:
        lam32 = np.float32(MERGE_LAMBDA[model])
        for W in MERGE_WORLDS:
            assert _merge_K(W) % 16 == 0 and _merge_K(W) % W == 0
            for i, kind in enumerate(MERGE_SETS):
                rec = merge_records(kind, W, D, T * C, float(lam32), seed=1000 * W + 10 * T * C + i)
                x = _merge_x(rec, T * C, lam32)
                assert ((x <= 80.0) | (x >= 200.0)).all(), (model, W, kind, x)
                assert (x.min(0) == 0).all()
                if kind.startswith("dominant"):
                    dom = 0 if kind == "dominant_first" else W - 1
                    assert (np.delete(x, dom, 0) >= 200.0).all() and (x[dom] == 0).all(), (model, W, kind)
                if kind == "equal":
                    assert (x == 0).all()
                eta, eta2 = rec[:, :, T * C + 1], rec[:, :, T * C + 2]
                assert (eta >= 1).all() and (eta <= _merge_K(W) // W).all() and (eta2 > 0).all() and (eta2 <= eta).all()


def _merge_reference(rec_z, TC, lam32, K):
    """float64 merge of the records [W][TC + 4] of one system -> (u*, its bound [TC], statistics, their bounds).

    u = 2^-24.  The engine forms s_b = det::exp(-fl(fl(rho_b - rho) * fl(1 / lambda))): three roundings in the argument
    (3u x_b absolute in the exponent) and <= 2 ulp of det::exp, so s_b carries d_b = 3u x_b + 4u relative (stats64's d_k).
    U[j] = sum_b s_b U_b[j] in fp32: every product rounds once and any order of W terms adds (W - 1) u, together W u relative to
    sum_b s_b |U_b[j]|; eta = sum_b s_b eta_b is accumulated in double, rounded to fp32 once, and the division rounds once:
      |u*_j - ref_j| <= sum_b s_b |U_b[j]| (d_b + W u) / eta + |ref_j| (sum_b s_b eta_b d_b / eta + 3u)
    Statistics, with the formulas and bound structure of test_kernel_sequence.stats64 (core/mppi_common.cu:1065-1081), the
    per-rollout sums replaced by the per-record ones: m = eta / K, m2 = sum_b s_b^2 eta2_b / K,
      e1 = sum_b s_b eta_b d_b / eta + 3u          (double accumulation; the narrowing, the division by K)
      e2 = sum_b s_b^2 eta2_b (2 d_b + u) / eta2 + 3u
    baseline exact, normaliser within SOFTMIN_RTOL."""
    u = UNIT
    W = rec_z.shape[0]
    r = rec_z.astype(np.float64)
    U, rho, eta_b, eta2_b = r[:, :TC], r[:, TC], r[:, TC + 1], r[:, TC + 2]
    lam = float(lam32)
    ref, rho_min, eta = merge_records_numpy(U, rho, eta_b, lam)
    x = (rho - rho_min) / lam
    s = np.exp(-x)
    d = 3 * u * x + 4 * u
    rel_eta = (s * eta_b * d).sum() / eta
    bound = (s[:, None] * np.abs(U) * (d[:, None] + W * u)).sum(0) / eta + np.abs(ref) * (rel_eta + 3 * u)
    eta2 = (s * s * eta2_b).sum()
    e1 = rel_eta + 3 * u
    e2 = (s * s * eta2_b * (2 * d + u)).sum() / eta2 + 3 * u
    mean, mean2 = eta / K, eta2 / K
    fe = -lam * np.log(mean) + rho_min
    var = lam * (mean2 - mean * mean)
    q = var / (mean * np.sqrt(K))
    mod = lam * (q + 0.5 * q * q)
    d_fe = lam * e1 + 8 * u * (lam * abs(np.log(mean)) + abs(rho_min))
    d_var = lam * (e2 * mean2 + (2 * e1 + u) * mean * mean) + 3 * u * abs(var)
    d_q = d_var / (mean * np.sqrt(K)) + abs(q) * (e1 + 6 * u)
    d_mod = lam * (1 + abs(q)) * d_q + 4 * u * abs(mod)
    vals = dict(baseline=rho_min, normalizer=eta, free_energy_mean=fe, free_energy_variance=var,
                free_energy_modified_variance=mod)
    bounds = dict(baseline=0.0, normalizer=SOFTMIN_RTOL * eta, free_energy_mean=d_fe, free_energy_variance=d_var,
                  free_energy_modified_variance=d_mod)
    return ref, bound, vals, bounds


def test_merge_reference_on_exact_inputs():
    """records whose merge is exact in any arithmetic: equal baselines, power-of-two weights"""
    TC, K = 3, 32
    rec = np.zeros((2, TC + 4), np.float32)
    rec[0] = [1.0, 2.0, -4.0, 5.0, 2.0, 1.5, 0.0]
    rec[1] = [3.0, -2.0, 8.0, 5.0, 6.0, 4.0, 0.0]
    ref, bound, vals, bounds = _merge_reference(rec, TC, np.float32(0.5), K)
    assert np.array_equal(ref, [0.5, 0.0, 0.5]) and vals["baseline"] == 5.0 and vals["normalizer"] == 8.0
    assert abs(vals["free_energy_mean"] - (-0.5 * np.log(8.0 / 32) + 5.0)) <= 1e-15
    assert abs(vals["free_energy_variance"] - 0.5 * (5.5 / 32 - (8.0 / 32) ** 2)) <= 1e-15
    assert (bound > 0).all() and (bound < 1e-6).all()
    # a record 300 lambda above the other has no say
    rec[1, TC] = 5.0 + 300 * 0.5
    ref, _, vals, _ = _merge_reference(rec, TC, np.float32(0.5), K)
    assert np.abs(ref - rec[0, :TC] / 2.0).max() < 1e-100 and abs(vals["normalizer"] - 2.0) < 1e-100


# ------------------------------------------------------------------ part A: GPU ---------------------------------------
def _exchange(ranks):
    """one caller-driven, host-staged iteration on all ranks: local -> gather on the host -> merge"""
    send = []
    for e in ranks:
        e.iterationLocal()
        send.append(e.readSendRecord())
    gathered = np.concatenate(send)
    for e in ranks:
        e.writeRecvRecords(gathered)
        e.iterationMerge()
    return gathered


def _run_sharded(case, K, W, T, philox):
    ctl = case["controller"]
    colored = ctl == "colored"
    mode = "philox" if philox else "injected"
    tag0 = "%s %s K=%d world=%d T=%d" % (case["id"], mode, K, W, T)
    Kl = K // W
    ranks = []
    orc = cfg = None
    try:
        for r in range(W):
            cfg, eng, o, _ = make_handles(dict(case, kw=dict(case["kw"], rank=r, world_size=W)), K, T)
            ranks.append(eng)
            orc = orc or o
        D, C = ranks[0].num_systems, ranks[0].CONTROL_DIM
        lam = cfg["lambda_"]
        sysnames = ["real_sys", "nominal_sys"][:D]
        x0 = np.tile(cfg["x0"], (D, 1))
        for r, e in enumerate(ranks):
            assert (e.num_rollouts_local, e.rollout_offset) == (Kl, r * Kl), "%s rank %d: owns %d rollouts from %d" % (
                tag0, r, e.num_rollouts_local, e.rollout_offset)
        noise = None
        if philox:
            for e in ranks:
                e.setSeed(PHILOX_SEED)
        else:
            noise = (host_spectrum(1, K, T, C, seed=K + T) if colored else host_noise(1, K, T, C, seed=K + T))[0]
            for r, e in enumerate(ranks):
                e.injectNoise(np.ascontiguousarray(noise[r * Kl:(r + 1) * Kl]))
        for e in ranks:
            e.uploadState(x0)
        chain = np.zeros((D, T, C), np.float32)  # the oracle's own mean, chained over the iterations
        drift = 0.0
        for g in range(PHILOX_ITERS if philox else 1):
            tag = "%s iteration %d" % (tag0, g)
            # the mean this iteration samples around: the engine's own, the same bits on every rank
            means = [e.getOptimalControlSeq() for e in ranks]
            for r in range(1, W):
                assert bits_equal(means[r], means[0], nan_equal=True), "%s rank %d: the mean before the iteration differs from rank 0's" % (tag, r)
            if philox:
                noise = po.philox_spectrum(PHILOX_SEED, g, K, T, C) if colored else po.philox_normal(PHILOX_SEED, g, K, T, C)
            eps = po.colored_noise(noise, *cfg["colored"], offset_t=1, flavour="engine") if colored else noise

            _exchange(ranks)

            # -------- which path ran
            for r, e in enumerate(ranks):
                info = e.getLaunchInfo()
                got = {k: info[k] for k in ("family", "block", "rows_in_hbm")}
                assert got == case["expect"], "%s rank %d: launched %s, the case expects %s" % (tag, r, got, case["expect"])
                assert not info["streamed_merge"], "%s rank %d: a sharded handle streamed the merge" % (tag, r)

            # -------- every rank's own rollouts against the oracle's slice, from the engine's own mean
            v_o = orc.set_gaussian_controls(means[0], eps, 1, g)
            costs_o, v_o = orc.rollout_costs(x0, means[0], v_o)
            costs_e = [e.getSampledCostSeq() for e in ranks]
            v_e = [e.getSampledControls() for e in ranks]
            for r in range(W):
                sl = slice(r * Kl, (r + 1) * Kl)
                assert np.isfinite(costs_e[r]).all(), "%s rank %d" % (tag, r)
                dc = ulp_diff(costs_e[r], costs_o[:, sl])
                assert int(dc.max()) == 0, "%s rank %d: costs differ from the oracle's slice by up to %d ulp, first at local rollout %d" % (
                    tag, r, int(dc.max()), int(np.argwhere(dc > 0)[0][-1]))
                dv = ulp_diff(v_e[r], v_o[:, sl]).reshape(D, Kl, -1).max(2)
                assert int(dv.max()) == 0, "%s rank %d: clamped samples differ from the oracle's slice by up to %d ulp, first at local rollout %d" % (
                    tag, r, int(dv.max()), int(np.argwhere(dv > 0)[0][-1]))

            # -------- the merged result
            chain = orc.iterate(x0, chain, eps, 1, g)
            us = [e.getOptimalControlSeq() for e in ranks]
            sts = [e.getStats() for e in ranks]
            for r in range(W):
                assert np.isfinite(us[r]).all(), "%s rank %d" % (tag, r)
                drift = max(drift, float(np.abs(us[r] - chain).max()))
                if not philox:
                    assert drift <= U_TOL, "%s rank %d: u* differs from the oracle's un-sharded iteration by %g" % (tag, r, drift)
                assert bits_equal(us[r], us[0], nan_equal=True), "%s rank %d: u* differs from rank 0's" % (tag, r)
                for name in sysnames:
                    a, b = stats_of(sts[r], name), stats_of(sts[0], name)
                    assert bits_equal(list(a.values()), list(b.values()), nan_equal=True), "%s rank %d: %s statistics %s, rank 0 has %s" % (
                        tag, r, name, a, b)

            # -------- float64, from the ranks' own dumps
            call, vall = np.concatenate(costs_e, axis=1), np.concatenate(v_e, axis=1)
            for z, name in enumerate(sysnames):
                want = softmin64(call[z], vall[z], lam)
                bound = SOFTMIN_RTOL * max(1.0, float(np.abs(want).max()))
                want_st, bound_st = stats64(call[z], lam)
                for r in range(W):
                    err = float(np.abs(us[r][z] - want).max())
                    assert err <= bound, "%s rank %d: system %d u* is %g from the float64 softmin of the ranks' samples (bound %g)" % (
                        tag, r, z, err, bound)
                    got = stats_of(sts[r], name)
                    for k in want_st:
                        assert abs(got[k] - want_st[k]) <= bound_st[k], "%s rank %d: %s %s = %r, float64 %r (bound %g)" % (
                            tag, r, name, k, got[k], want_st[k], bound_st[k])
        if philox:
            bound = FUSED_DRIFT.get((case["id"], "philox"), U_TOL)
            assert drift <= bound, "%s: u* differs from the oracle's un-sharded chained iterations by up to %g (bound %g)" % (
                tag0, drift, bound)
    finally:
        for e in ranks:
            e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", SHARDED_CASES, ids=[c["id"] for c in SHARDED_CASES])
def test_sharded_matrix(gpu, case):
    for K, W, T in _shapes(case):
        _run_sharded(case, K, W, T, philox=False)
    _run_sharded(case, *PHILOX_SHAPE, philox=True)


# ------------------------------------------------------------------ part B: GPU ---------------------------------------
def _merge_cfg(model, D, W, T):
    K = _merge_K(W)
    if model == "cartpole":
        cfg = cartpole_cfg(K=K, T=T, lambda_=MERGE_LAMBDA[model])
        cfg["D"] = D
        return cfg
    return di_cfg(K=K, T=T, tube=D == 2, lambda_=MERGE_LAMBDA[model])


def _merge_once(eng, rec, D):
    eng.writeRecvRecords(rec)
    eng.iterationMerge()
    st = eng.getStats()
    return eng.getOptimalControlSeq(), [stats_of(st, n) for n in ["real_sys", "nominal_sys"][:D]]


@pytest.mark.gpu
@pytest.mark.parametrize("problem", MERGE_PROBLEMS, ids=[p[0] for p in MERGE_PROBLEMS])
def test_gathered_merge_on_written_records(gpu, problem):
    tag0, model, D, C, T = problem
    TC = T * C
    lam32 = np.float32(MERGE_LAMBDA[model])
    for W in MERGE_WORLDS:
        cfg = _merge_cfg(model, D, W, T)
        K = cfg["K"]
        eng = make_engine(cfg, tube=D == 2, rank=0, world_size=W)
        try:
            assert eng.exchangeBuffers()[2] == D * (TC + 4), tag0
            # one ordinary local iteration first, so that the handle is in the state a merge is normally called in
            eng.uploadState(np.tile(cfg["x0"], (D, 1)))
            eng.iterationLocal()
            for i, kind in enumerate(MERGE_SETS):
                tag = "%s world=%d %s" % (tag0, W, kind)
                rec = merge_records(kind, W, D, TC, float(lam32), seed=1000 * W + 10 * TC + i)
                u, st = _merge_once(eng, rec, D)
                worst = dict(u=0.0)
                for z in range(D):
                    ref, bound, vals, bounds = _merge_reference(rec[:, z], TC, lam32, K)
                    err = np.abs(u[z].reshape(-1).astype(np.float64) - ref)
                    j = int(np.argmax(err / bound))
                    worst["u"] = max(worst["u"], float(err[j] / bound[j]))
                    assert (err <= bound).all(), "%s: system %d u*[%d] = %r, float64 merge %r: off by %g, bound %g" % (
                        tag, z, j, u[z].reshape(-1)[j], ref[j], err[j], bound[j])
                    for k in vals:
                        e = abs(st[z][k] - vals[k])
                        if bounds[k] > 0:
                            worst[k] = max(worst.get(k, 0.0), float(e / bounds[k]))
                        assert e <= bounds[k], "%s: system %d %s = %r, float64 %r (bound %g)" % (
                            tag, z, k, st[z][k], vals[k], bounds[k])
                print("merge error / bound  %s: %s" % (tag, "  ".join("%s %.3f" % kv for kv in worst.items())))
                if kind.startswith("dominant"):
                    # every other record's scale factor is exactly 0: what those records hold cannot reach the result
                    dom = 0 if kind == "dominant_first" else W - 1
                    rec2 = rec.copy()
                    for b in range(W):
                        if b != dom:
                            rec2[b, :, :TC] = 1e30
                    u2, st2 = _merge_once(eng, rec2, D)
                    assert bits_equal(u2, u, nan_equal=True), "%s: u* changed when the underflowed records' U became 1e30" % tag
                    for z in range(D):
                        assert bits_equal(list(st2[z].values()), list(st[z].values()), nan_equal=True), "%s: system %d statistics changed: %s -> %s" % (
                            tag, z, st[z], st2[z])
        finally:
            eng.close()


# ------------------------------------------------------------------ part C: GPU ---------------------------------------
@pytest.mark.gpu
def test_caller_driven_iteration_refuses_tsallis_weights_on_a_sharded_handle(gpu):
    """Tsallis weights need the global baseline before any weight, i.e. two exchanges per iteration: the caller-driven pair has
    one, and mppi_iteration_local says so instead of merging weights taken under per-rank baselines"""
    cfg = colored_cartpole(K=128, T=8)
    eng = make_engine(cfg, rank=1, world_size=2)
    try:
        eng.setColoredMPPIParams(gamma=400.0, r_exp=1.7)
        eng.uploadState(cfg["x0"])
        with pytest.raises(m.MPPIError) as e:
            eng.iterationLocal()
        assert e.value.status == m.MPPI_ERR_UNSUPPORTED, e.value.status
        # without them the same handle runs
        eng.setColoredMPPIParams(gamma=0.0, r_exp=0.0)
        eng.iterationLocal()
        assert np.isfinite(eng.readSendRecord()).all()
    finally:
        eng.close()
