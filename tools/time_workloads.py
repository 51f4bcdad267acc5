#!/usr/bin/env python3
"""Times optimisation iterations of the registered workloads for several block shapes (HIP events on the engine's
stream).  Usage: python tools/time_workloads.py [cartpole|autorally|autorally-robust|di|lstm|racer|quadrotor|quadrotor-map|quadrotor-volume|nln|nln-gaussian] ...
(nln / nln-gaussian: the Cartpole pipeline kernel at K = 16384, T = 100 with the NLN and with the Gaussian sampler, one workload
each so that a kernel trace of either holds one rollout kernel; not part of the default set.
quadrotor: the reference's hover configuration at 2048 x 150 and 16384 x 150, each beside the double integrator at the same K and T
— an analytic model on the same kernels, as the yardstick; not part of the default set either: the model's registration unit is
examples/quadrotor_model/quadrotor_model.hip, built and loaded here.
quadrotor-map: QuadrotorMapCost on the three-gate course and track map of examples/templated_quadrotor_map.hip at the same two
sizes, registration unit examples/quadrotor_model/quadrotor_map_model.hip; an argument ending in .so is another build of that
unit to load in its place, for an A/B of two builds of the cost.
quadrotor-volume: QuadrotorVolumeCost (QuadrotorQuadraticCost + a 64 x 64 x 16 clearance volume through ThreeDTextureHelper) at
K = 16384, T = 100, beside "quadrotor_map" (its course and track map) and "quadrotor" (the hover cost) at the same K, T and dt in
the same run; registration unit examples/quadrotor_model/quadrotor_volume_model.hip.
autorally-robust: "autorally_nn_robust" (ARRobustCost on a four-channel 600 x 600 map over the standard track map's extent) at
K = 16384, T = 150 — the vanilla iteration on the default MFMA shape, fused and role-pipelined, and Robust MPPI's computeControl
(wall clock around the call, which returns after the control is on the host) — each beside "autorally_nn" with ARStandardCost in
the same run, as the yardstick; registration unit examples/autorally_robust_model/autorally_robust_model.hip, or an argument ending
in .so)
linearize / feedback: wall clock of mppi_linearize_trajectory / mppi_compute_feedback on Cartpole T = 100 and AutoRally-NN T = 150;
not part of the default set.
replay: wall clock of mppi_top_rollouts(32) and mppi_replay_rollouts(33 rows) next to mppi_linearize_trajectory on Cartpole
K = 16384, T = 100; not part of the default set.
evaluate: wall clock of mppi_evaluate_controls on n = 16384 caller-supplied control sequences, Cartpole T = 100 and AutoRally-NN
T = 150 (both lane forms); not part of the default set.)"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
from common import autorally_cfg, bicycle_lstm_cfg, cartpole_cfg, di_cfg, make_engine  # noqa: E402


def run(name, cfg, shapes, n=100, setup=None, **kw):
    for sh in shapes:
        bx, by = sh[0], sh[1]
        variant = sh[2] if len(sh) > 2 else 0
        try:
            eng = make_engine(cfg, block_x=bx, block_y=by, kernel_variant=variant, **kw)
            if setup:
                setup(eng)
        except Exception as e:  # noqa: BLE001
            print(name, (bx, by), "skip:", e)
            continue
        x0 = np.tile(cfg["x0"], (cfg["D"], 1))
        eng.uploadState(x0)
        eng.optimize(20)
        tot, roll = eng.timeIterations(n)
        print("%-10s K=%d T=%d shape=(%d,%d,%d) variant=%d: iteration %.1f us, rollout kernel %.1f us" %
              (name, cfg["K"], cfg["T"], bx, by, cfg["D"], variant, tot / n * 1e3, roll / n * 1e3), flush=True)
        eng.close()


which = sys.argv[1:] or ["cartpole", "autorally", "di", "lstm", "racer"]
if "cartpole" in which:
    run("cartpole", cartpole_cfg(K=16384, T=100), [(64, 1, 1), (64, 1, 2), (32, 1)])
    run("cartpole", cartpole_cfg(K=2048, T=100), [(64, 1)])
if "nln" in which or "nln-gaussian" in which:
    import mppi_generic_amd as m  # noqa: E402
    nln_cfg = cartpole_cfg(K=16384, T=100)
    nln_cfg["std_dev"] = [0.8]  # exp(std_dev z') as the log-normal factor: 5.0 would pin every sample at the control range
    if "nln-gaussian" in which:
        run("cartpole", nln_cfg, [(64, 1, 2)], n=300)
    if "nln" in which:
        run("cartpole+nln", nln_cfg, [(64, 1, 2)], n=300, sampler=m.MPPI_SAMPLER_NLN)
if "autorally" in which:
    # (0, 0, v): the model's default shape — (64, 4), or (64, 8) in the eight-lanes-per-rollout A/B build
    run("autorally", autorally_cfg(K=16384, T=150, lambda_=1.0), [(0, 0, 1), (0, 0, 2), (32, 4), (32, 8)], n=30)
if "di" in which:
    run("di-tube", di_cfg(K=8192, T=150, tube=True), [(64, 1, 1), (0, 0, 0), (32, 1, 2)])
    # Tube with colored noise: the fused (64, 1, 2) kernel (at T = 150 the rows of 2 x 64 slots go to HBM), beside the Gaussian lines above
    run("di-tube+colored", di_cfg(K=8192, T=150, tube=True), [(64, 1, 1)], sampler=1, setup=lambda e: e.setColoredNoiseParams([1.0, 1.0]))
if "lstm" in which:
    cfg = bicycle_lstm_cfg(K=65536, T=200, lambda_=1.0)
    run("lstm", cfg, [(0, 0, 1), (0, 0, 2)], n=10)
    cfg["colored"] = ([1.0, 1.0], 0.97, 0.0)
    run("lstm+colored", cfg, [(0, 0, 1), (0, 0, 2)], n=10)
    cfg = cartpole_cfg(K=16384, T=100)
    cfg["colored"] = ([1.0], 0.97, 0.0)
    run("cartpole+colored", cfg, [(64, 1, 1), (64, 1, 2)], n=50)
if "racer" in which:
    from common import racer_cfg  # noqa: E402
    from racer_cfgs import elevation_cfg, steering_cfg  # noqa: E402
    run("racer", racer_cfg(K=16384, T=100), [(64, 1, 1), (64, 1, 2)], n=50)
    run("racer-elev", elevation_cfg(K=16384, T=100), [(64, 1, 1), (64, 1, 2), (64, 4, 1), (64, 4, 2)], n=50)
    run("racer-flat", elevation_cfg(K=16384, T=100, with_map=False), [(64, 1, 2)], n=50)
    run("racer-lstm", steering_cfg(K=16384, T=100), [(64, 1, 1), (64, 4, 1), (64, 4, 2)], n=50)
    from racer_cfgs import suspension_cfg  # noqa: E402
    run("racer-suspension", suspension_cfg(K=16384, T=100), [(64, 1, 1), (64, 4, 1), (64, 4, 2)], n=30)
    from racer_cfgs import uncertainty_cfg  # noqa: E402
    run("racer-uncertainty", uncertainty_cfg(K=16384, T=100), [(64, 1, 1), (64, 4, 1), (64, 4, 2)], n=30)
    cfg = steering_cfg(K=16384, T=100)
    cfg["colored"] = ([1.0, 1.0], 0.97, 0.0)
    run("racer-lstm+colored", cfg, [(0, 0, 0)], n=30)
if "quadrotor" in which:
    import mppi_generic_amd as m  # noqa: E402
    import quadrotor_oracle  # noqa: E402
    from test_quadrotor import hover_cfg  # noqa: E402
    quadrotor_oracle.load_model(m)
    for K in (2048, 16384):
        cfg = hover_cfg()
        cfg["K"] = K
        run("quadrotor", cfg, [(64, 1, 1), (64, 1, 2), (32, 4, 1)], n=50)
        run("di", di_cfg(K=K, T=150, tube=False), [(64, 1, 1), (64, 1, 2)], n=50)
if "quadrotor-map" in which:
    import mppi_generic_amd as m  # noqa: E402
    import quadrotor_map_oracle  # noqa: E402
    from test_templated_quadrotor_map import course_map, course_params  # noqa: E402
    other = [a for a in which if a.endswith(".so")]
    if other:
        assert m.load_library().mppi_load_plugin(os.path.abspath(other[0]).encode()) == m.MPPI_OK
    else:
        quadrotor_map_oracle.load_model(m)
    values, frame = course_map()
    x0 = np.zeros(13, np.float32)
    x0[2], x0[6] = 1.0, 1.0
    for K in (2048, 16384):
        cfg = dict(model="quadrotor_map", K=K, T=150, D=1, dt=0.02, lambda_=5.0, alpha=0.0, num_iters=1, dyn=m.QuadrotorDynamicsParams(),
                   cost=course_params(), ranges=None, std_dev=[0.5, 0.5, 0.5, 2.0], control_cost_coeff=[1.0] * 4, x0=x0,
                   blobs={"costmap_transform": frame, "costmap": values})
        run("quadrotor-map", cfg, [(64, 1, 1), (64, 1, 2), (32, 4, 1)], n=50)
if "quadrotor-volume" in which:
    import mppi_generic_amd as m  # noqa: E402
    import quadrotor_map_oracle  # noqa: E402
    import quadrotor_oracle  # noqa: E402
    import texture3d_oracle  # noqa: E402
    from test_quadrotor import hover_cfg  # noqa: E402
    from test_templated_quadrotor_map import course_map, course_params  # noqa: E402
    for loader in (texture3d_oracle, quadrotor_map_oracle, quadrotor_oracle):
        loader.load_model(m)
    K, T = 16384, 100
    x0 = np.zeros(13, np.float32)
    x0[2], x0[6] = 1.0, 1.0
    # a pillar at (3, 0) in 0.125 m cells over x in [-1, 7), y in [-4, 4), z in [0, 2): the rollouts from (0, 0, 1) cross cells and layers
    X, Y = np.meshgrid(-1 + 0.125 * (np.arange(64) + 0.5), -4 + 0.125 * (np.arange(64) + 0.5))
    layer = np.maximum(0.0, 1.0 - np.hypot(X - 3.0, Y) / 2.0).astype(np.float32)
    volume = np.ascontiguousarray(np.broadcast_to(layer[None], (16, 64, 64)) * np.linspace(1.0, 0.5, 16, dtype=np.float32)[:, None, None])
    vol_cost = m.QuadrotorVolumeCostParams()
    hover = hover_cfg()
    for f, _ in m.QuadrotorQuadraticCostParams._fields_:
        setattr(vol_cost, f, getattr(hover["cost"], f))
    base = dict(K=K, T=T, D=1, dt=0.02, lambda_=5.0, alpha=0.0, num_iters=1, dyn=m.QuadrotorDynamicsParams(), ranges=None,
                std_dev=[0.5, 0.5, 0.5, 2.0], control_cost_coeff=[1.0] * 4, x0=x0)
    values, frame = course_map()
    for name, cfg in (("quadrotor-volume", dict(base, model="quadrotor_volume", cost=vol_cost,
                                                blobs={"cost_volume_transform": texture3d_oracle.frame15([-1, -4, 0], np.eye(3), [0.125] * 3),
                                                       "cost_volume": volume})),
                      ("quadrotor-map", dict(base, model="quadrotor_map", cost=course_params(),
                                             blobs={"costmap_transform": frame, "costmap": values})),
                      ("quadrotor", dict(base, model="quadrotor", cost=hover["cost"]))):
        run(name, cfg, [(64, 1, 1), (64, 1, 2)], n=50)
if "autorally-robust" in which:
    import time  # noqa: E402
    import mppi_generic_amd as m  # noqa: E402
    import ar_robust_oracle  # noqa: E402
    from common import SEED, standard_track_map  # noqa: E402
    other = [a for a in which if a.endswith(".so")]
    if other:
        assert m.load_library().mppi_load_plugin(os.path.abspath(other[0]).encode()) == m.MPPI_OK
    else:
        ar_robust_oracle.load_model(m)
    std = autorally_cfg(K=16384, T=150, lambda_=1.0)
    track, bounds = standard_track_map()
    # boundary constraint rising to 1 away from the centre line, the standard map as the track position, 4 m/s, heading 0
    texels = ar_robust_oracle.interleave([np.clip(track / 10.0, 0.0, 1.0), track, np.full_like(track, 4.0), np.zeros_like(track)])
    cost = m.ARRobustCostParams()
    cost.setTransformFromBounds(*bounds)
    cost.heading_coeff = 5.0
    rob = dict(std, model="autorally_nn_robust", cost=cost, blobs={"dynamics_weights": std["blobs"]["dynamics_weights"], "costmap": texels})
    for name, cfg in (("ar-robust", rob), ("autorally", std)):
        run(name, cfg, [(0, 0, 1), (0, 0, 2)], n=30)
    gains = np.random.default_rng(5).uniform(-0.3, 0.3, (150, 7, 2)).astype(np.float32)
    for name, cfg in (("ar-robust", rob), ("autorally", std)):
        eng = m.RobustMPPIController(cfg["model"], cfg["K"], cfg["T"], cfg["dt"], cfg["lambda_"], cfg["alpha"], 1, seed=SEED)
        eng.setCostParams(cfg["cost"])
        for blob, arr in cfg["blobs"].items():
            eng.setModelBlob(blob, arr)
        eng.setControlRanges(cfg["ranges"])
        eng.setSamplingParams(cfg["std_dev"], [0.2, 0.1], 0.01, 1.0)
        eng.setRMPPIParams(1000.0, 9, 32)
        eng.updateImportanceSamplingControl(cfg["x0"], 1)
        eng.setFeedbackGains(gains)
        for _ in range(5):
            eng.computeControl(cfg["x0"], 1)
        t0 = time.perf_counter()
        for _ in range(30):
            eng.computeControl(cfg["x0"], 1)
        us = (time.perf_counter() - t0) / 30 * 1e6
        print("%-10s K=%d T=%d Robust computeControl %.1f us (%s)" % (name, cfg["K"], cfg["T"], us, eng.getLaunchInfo()["family"]), flush=True)
        eng.close()
if "linearize" in which:
    # mppi_linearize_trajectory next to the same handle's computeControl: wall time of the whole call (launch, two copies back,
    # one synchronisation), median and spread over repeated calls after warm-up.  5000 calls each: a timed window of 0.2 - 1.2 s,
    # so that clock ramp and scheduler noise are a small part of it.  The kernel's own time is not in these figures; take it
    # from a kernel trace of this mode, in a run of its own.
    import time  # noqa: E402
    for name, cfg in (("cartpole", cartpole_cfg(K=16384, T=100)), ("autorally", autorally_cfg(K=16384, T=150, lambda_=1.0))):
        eng = make_engine(cfg)
        for _ in range(200):
            eng.computeControl(cfg["x0"], 1)
            eng.computeGradTrajectory()

        def timed(fn, n=5000):
            t = []
            for _ in range(n):
                t0 = time.perf_counter()
                fn()
                t.append((time.perf_counter() - t0) * 1e6)
            return np.percentile(t, [50, 10, 90])

        cc = timed(lambda: eng.computeControl(cfg["x0"], 1))
        eng.getTargetStateSeq()
        lin = timed(eng.computeGradTrajectory)
        print("%-10s K=%d T=%d computeControl %.1f us (p10 %.1f, p90 %.1f); linearize_trajectory %.1f us (p10 %.1f, p90 %.1f)"
              % ((name, cfg["K"], cfg["T"]) + tuple(cc) + tuple(lin)), flush=True)
        eng.close()
if "feedback" in which:
    # mppi_compute_feedback (linearizeKernel + ddpBackwardKernel, the gains and the status back, one synchronisation) next to
    # mppi_linearize_trajectory on the same handle: wall time of the whole call, median and p10 / p90 over 5000 calls after
    # warm-up, as the linearize mode above.  The kernels' own times are not in these figures; take them from a kernel trace of
    # this mode, in a run of its own.
    import time  # noqa: E402
    for name, cfg in (("cartpole", cartpole_cfg(K=16384, T=100)), ("autorally", autorally_cfg(K=16384, T=150, lambda_=1.0))):
        eng = make_engine(cfg)
        for _ in range(200):
            eng.computeControl(cfg["x0"], 1)
            eng.computeGradTrajectory()
            eng.computeFeedback()

        def timed(fn, n=5000):
            t = []
            for _ in range(n):
                t0 = time.perf_counter()
                fn()
                t.append((time.perf_counter() - t0) * 1e6)
            return np.percentile(t, [50, 10, 90])

        eng.getTargetStateSeq()
        lin = timed(eng.computeGradTrajectory)
        fb = timed(eng.computeFeedback)
        print("%-10s K=%d T=%d linearize_trajectory %.1f us (p10 %.1f, p90 %.1f); compute_feedback %.1f us (p10 %.1f, p90 %.1f)"
              % ((name, cfg["K"], cfg["T"]) + tuple(lin) + tuple(fb)), flush=True)
        eng.close()
if "replay" in which:
    # mppi_top_rollouts(n = 32) and mppi_replay_rollouts(n = 33: the optimal sequence and the 32 best rollouts) next to
    # mppi_linearize_trajectory on the same handle (Cartpole K = 16384, T = 100, saved samples): wall time of the whole call (launch,
    # copies, one synchronisation), median and p10 / p90 over 5000 calls after warm-up, as the linearize mode above.  The kernels'
    # own times are not in these figures; take them from a kernel trace of this mode, in a run of its own.
    import time  # noqa: E402
    cfg = cartpole_cfg(K=16384, T=100)
    eng = make_engine(cfg, save_samples=True)
    for _ in range(200):
        eng.computeControl(cfg["x0"], 1)
        eng.computeGradTrajectory()
        rows = np.concatenate([np.array([-1], np.int32), eng.top_rollouts(32)[0]])
        eng.replay_rollouts(rows)

    def timed(fn, n=5000):
        t = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e6)
        return np.percentile(t, [50, 10, 90])

    eng.getTargetStateSeq()
    lin = timed(eng.computeGradTrajectory)
    top = timed(lambda: eng.top_rollouts(32))
    rep = timed(lambda: eng.replay_rollouts(rows))
    print("cartpole   K=%d T=%d linearize_trajectory %.1f us (p10 %.1f, p90 %.1f); top_rollouts(32) %.1f us (p10 %.1f, p90 %.1f); "
          "replay_rollouts(33) %.1f us (p10 %.1f, p90 %.1f)" % ((cfg["K"], cfg["T"]) + tuple(lin) + tuple(top) + tuple(rep)), flush=True)
    eng.close()
if "evaluate" in which:
    # mppi_evaluate_controls on n = 16384 control sequences of the caller's own: Cartpole T = 100 (one lane per row) and AutoRally-NN
    # T = 150 on its one-rollout-per-wave form and, with MPPI_AMD_FINALIZE_FORM=rep, on its replicated lanes.  Wall time of the whole
    # call — the copy of the rows from pageable host memory (6.6 MB / 19.7 MB), the launch, the copy of the results back, one
    # synchronisation — median and p10 / p90 over 200 calls after warm-up; and of a call with n = 64 rows on the same handle, which
    # is the fixed part.  The kernel's own time is not in these figures; take it from a kernel trace of this mode, in a run of its own.
    import time  # noqa: E402

    def timed(fn, n=200):
        t = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e6)
        return tuple(np.percentile(t, [50, 10, 90]))

    for name, cfg, form in (("cartpole", cartpole_cfg(K=16384, T=100), None),
                            ("autorally", autorally_cfg(K=16384, T=150, lambda_=1.0), None),
                            ("autorally", autorally_cfg(K=16384, T=150, lambda_=1.0), "rep")):
        if form:
            os.environ["MPPI_AMD_FINALIZE_FORM"] = form
        eng = make_engine(cfg)
        C_ = eng.CONTROL_DIM
        u = np.random.default_rng(1).uniform(-1.0, 1.0, (16384, cfg["T"], C_)).astype(np.float32)
        for _ in range(20):
            eng.evaluate_controls(cfg["x0"], u)
        big = timed(lambda: eng.evaluate_controls(cfg["x0"], u))
        small = timed(lambda: eng.evaluate_controls(cfg["x0"], u[:64]))
        print("%-10s n=16384 T=%d form=%s evaluate_controls %.1f us (p10 %.1f, p90 %.1f); n=64: %.1f us (p10 %.1f, p90 %.1f)"
              % ((name, cfg["T"], form or "default") + big + small), flush=True)
        eng.close()
        os.environ.pop("MPPI_AMD_FINALIZE_FORM", None)
