#!/usr/bin/env python3
"""Times optimisation iterations of the registered workloads for several block shapes (HIP events on the engine's
stream).  Usage: python tools/time_workloads.py [cartpole|autorally|di|lstm|racer|quadrotor|quadrotor-map|nln|nln-gaussian] ...
(nln / nln-gaussian: the Cartpole pipeline kernel at K = 16384, T = 100 with the NLN and with the Gaussian sampler, one workload
each so that a kernel trace of either holds one rollout kernel; not part of the default set.
quadrotor: the reference's hover configuration at 2048 x 150 and 16384 x 150, each beside the double integrator at the same K and T
— an analytic model on the same kernels, as the yardstick; not part of the default set either: the model's registration unit is
examples/quadrotor_model/quadrotor_model.hip, built and loaded here.
quadrotor-map: QuadrotorMapCost on the three-gate course and track map of examples/templated_quadrotor_map.hip at the same two
sizes, registration unit examples/quadrotor_model/quadrotor_map_model.hip; an argument ending in .so is another build of that
unit to load in its place, for an A/B of two builds of the cost)"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
from common import autorally_cfg, bicycle_lstm_cfg, cartpole_cfg, di_cfg, make_engine  # noqa: E402


def run(name, cfg, shapes, n=100, **kw):
    for sh in shapes:
        bx, by = sh[0], sh[1]
        variant = sh[2] if len(sh) > 2 else 0
        try:
            eng = make_engine(cfg, block_x=bx, block_y=by, kernel_variant=variant, **kw)
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
