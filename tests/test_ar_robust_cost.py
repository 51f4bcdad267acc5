"""ARRobustCost (the AutoRally cost of the reference's Robust MPPI set-up, over a four-channel track map) and its model,
registered as "autorally_nn_robust".

CPU: the shipped class built for the host (tests/ar_robust_oracle/robust_cost_host.hip) against the reference's own known answers
(getStabilizingCostTest, the two costmap tests on the regenerated robust test map), against hand-derived answers, one per branch,
and against the CPU restatement (tests/ar_robust_oracle/ar_robust_oracle.cpp) bit for bit; the restatement against an independent
float64 numpy restatement; the parameter block's layout in C, C++ and Python; the registration.
GPU: a branch census on the restatement first; then every kernel form of the registration — Vanilla, Tube and Robust — against the
restatement (costs 0 ulp, clamped samples 0 ulp, u* within 1e-5; bit for bit in reference-order reduction), the .npz loader, and
what the "costmap" blob refuses on a 1- and on a 4-channel cost.
"""
import ctypes as C

import numpy as np
import pytest

import mppi_generic_amd as m
import pyoracle as po
import ar_robust_oracle as ar
from common import PHILOX_SEED, SEED, U_TOL, autorally_cfg, host_noise, make_engine, ulp_diff
from restate64 import bits, bits_equal

REL_TOL = 1e-4  # the quadrotor tests' bar against float64 (the reference's own rollout tolerance)
MARGIN = 1e-3   # every state compared with float64 is at least this far from every threshold and texel boundary
MAX_COST = np.float32(1e16)
ATAN_ULP = 3    # det::atan's documented bound against float64 (include/mppi_amd/det_math.h)


@pytest.fixture(scope="module")
def robust_model(lib):
    """the registration unit is examples/autorally_robust_model/autorally_robust_model.hip: built on its own and loaded with
    mppi_load_plugin at test time — and taken out of the process-wide registry again when this module is done: the kernel-form
    test files that run later in a session enumerate the registry and want a configuration builder for every name in it"""
    lib_ = ar.load_model(m)
    yield lib_
    assert lib_.mppi_unregister_model(b"autorally_nn_robust", m.MPPI_SAMPLER_GAUSSIAN) == m.MPPI_OK
    assert "autorally_nn_robust" not in m.list_models()


@pytest.fixture(scope="module")
def host():
    return ar.HostCost()


def state(x=0.0, y=0.0, yaw=0.0, roll=0.0, vx=0.0, vy=0.0, yaw_rate=0.0):
    return np.array([x, y, yaw, roll, vx, vy, yaw_rate], np.float32)


# ------------------------------------------------------------------ CPU: the reference's getStabilizingCostTest ---------
def test_reference_stabilizing_cost(host):
    """tests/cost_functions/autorally_robust_cost_test.cu getStabilizingCostTest: max_slip_ang 1.25, crash_coeff 10000, slip_coeff
    10.  (vx, vy) = (0.24, 0) -> 0 exactly; (1, 1) -> 10 atan 1; (1, 10), and the same with roll 1.5 -> 10 atan 10 + 10000 (the
    slip is past max_slip_ang: the whole ramp).
    Two bars.  Against float64 10 atan(.) (+ 10000): det::atan's documented 3 ulp, scaled by 10, plus one rounding of the product
    and one of the sum, in ulp of the result.  Against the reference's own literals (0.785398 * 10, 1.4711 * 10 + 10000), which
    are six-digit decimals — a correctly rounded atan is itself 4 float ulp from the first — 1e-6 relative."""
    p = m.ARRobustCostParams()
    p.max_slip_ang, p.crash_coeff, p.slip_coeff = 1.25, 10000, 10
    host.set_cost_params(p)
    assert bits(host.stabilizing(state(vx=0.24, vy=0.0))) == bits(np.float32(0.0))
    for s, exact, literal in ((state(vx=1, vy=1), 10 * np.arctan(1.0), 0.785398 * 10),
                              (state(vx=1, vy=10), 10 * np.arctan(10.0) + 10000, 1.4711 * 10 + 10000),
                              (state(vx=1, vy=10, roll=1.5), 10 * np.arctan(10.0) + 10000, 1.4711 * 10 + 10000)):
        got = float(host.stabilizing(s))
        slip_term = exact - (10000 if exact > 10000 else 0)
        # 3 ulp of atan's value carried through the product (ulp of the product's binade may be the same or larger: the
        # absolute error of atan times 10), half an ulp for the product, half an ulp of the result for the sum
        bound = 10 * ATAN_ULP * np.spacing(np.float32(slip_term / 10)) + 0.5 * np.spacing(np.float32(slip_term)) + \
            0.5 * np.spacing(np.float32(exact))
        print("stabilizing cost %r: %.9g, float64 %.9g (bound %.3g), literal %.9g" % (s[3:6].tolist(), got, exact, bound, literal))
        assert abs(got - exact) <= bound, (s, got, exact)
        assert abs(got - literal) <= 1e-6 * literal, (s, got, literal)
    assert host.L.robust_cost_max_cost_value() == MAX_COST
    assert host.L.robust_cost_traits() == (1 | 2 | (4 << 4))  # barrier-free, kernarg-viewable, COSTMAP_CHANNELS == 4


# ------------------------------------------------------------------ CPU: the reference's costmap known answers ----------
ROBUST_MAP_BOUNDS = (-25.0, 45.0, -50.0, 5.0)


def robust_track_channels():
    """the four channels of the reference's `track_map_robust.npz` (scripts/autorally/test/generateTestMaps.py:76-109),
    regenerated: 70 m x 55 m at 20 px/m.  The generator fills (1400, 1100) arrays at [i, j] with x = j / 20, y = i / 20 —
    channel0 1 for x > 50 or x < 15, 0.6 for x > 40 or x < 25, else 0; channel1 |55 / 2 - y| + x / 70; channel2 x; channel3
    atan2(y, x) — and flattens them; the loader reads each flat array as width 1400, height 1100."""
    i = np.arange(1400, dtype=np.float64)[:, None] + np.zeros((1, 1100))
    j = np.arange(1100, dtype=np.float64)[None, :] + np.zeros((1400, 1))
    x, y = j / 20.0, i / 20.0
    c0 = np.where((x > 50) | (x < 15), 1.0, np.where((x > 40) | (x < 25), 0.6, 0.0))
    chans = (c0, np.abs(55 / 2.0 - y) + x / 70, x, np.arctan2(y, x))
    return [c.astype(np.float32).reshape(-1).reshape(1100, 1400) for c in chans]


@pytest.fixture(scope="module")
def robust_track():
    t = ar.interleave(robust_track_channels())
    t.setflags(write=False)
    return t


def reference_fixture_params(desired_speed):
    """the reference fixture's parameters (autorally_robust_cost_test.cu:20-28)"""
    p = m.ARRobustCostParams()
    p.boundary_threshold, p.crash_coeff, p.track_slop, p.speed_coeff, p.heading_coeff = 0.0, 10000, 0.0, 10, 20
    p.desired_speed = desired_speed
    p.setTransformFromBounds(*ROBUST_MAP_BOUNDS)
    return p


def costmap_terms64(texel_front, texel_back, p, vx, sin_yaw):
    c = min(1.0, max(float(texel_front[0]), float(texel_back[0])))
    total = 0.0
    if c >= p.boundary_threshold:
        total += (c - p.boundary_threshold) / (1.0 - p.boundary_threshold) * p.crash_coeff
    if texel_front[1] > p.track_slop:
        total += p.track_coeff * float(texel_front[1])
    total += p.speed_coeff * abs(vx - (float(texel_front[2]) if p.desired_speed == -1 else p.desired_speed))
    return total + p.heading_coeff * abs(sin_yaw + float(texel_front[3]))


def test_reference_costmap_known_answers(host, robust_track):
    """getCostmapCostSpeedMapTest / SpeedNoMapTest: state (3, 0, pi/2, 0, 2, 1, 0.1) on the robust test map; the reference expects
    11629.229 with desired_speed = -1 and 11349.729 with desired_speed = 10.
    At the literal state both query points sit exactly on texel boundaries (u 1400 = 560.0, v 1100 = 1010.0 and 990.0).  The floor
    rule there picks (560, 1010) and (560, 990) and gives 11785.356 / 11355.356; the reference's numbers come from (559, 1009) and
    (559, 989) — the texture unit's boundary effect DESIGN.md §3 records for ARStandardCost.  Asserted: the state moved by -0.013 m
    in x and y (one texel lower, off the boundaries) gives the reference's numbers within EXPECT_FLOAT_EQ's 4 ulp; the literal state
    gives the floor rule's numbers; and the two differ by exactly the texel values involved."""
    host.set_costmap(robust_track)
    literal = state(3, 0, np.pi / 2, 0, 2, 1, 0.1)
    moved = literal - state(0.013, 0.013)
    for desired_speed, want_ref, want_floor in ((-1, 11629.229, 11785.356), (10, 11349.729, 11355.356)):
        p = reference_fixture_params(desired_speed)
        host.set_cost_params(p)
        got_moved, got_literal = host.terms(moved)[1], host.terms(literal)[1]
        print("desired_speed %g: moved %.9g (reference %.9g), literal %.9g (floor rule %.9g)" % (desired_speed, got_moved, want_ref,
                                                                                               got_literal, want_floor))
        assert ulp_diff(got_moved, np.float32(want_ref)) <= 4, (desired_speed, got_moved)
        assert ulp_diff(got_literal, np.float32(want_floor)) <= 4, (desired_speed, got_literal)
        # which texels: the literal state's on the boundary rows / column, the moved state's one lower in both
        front, back = (3.0, 0.5), (3.0, -0.5)
        assert host.texel_index(*front) == 1010 * 1400 + 560 and host.texel_index(*back) == 990 * 1400 + 560
        assert host.texel_index(front[0] - 0.013, front[1] - 0.013) == 1009 * 1400 + 559
        assert host.texel_index(back[0] - 0.013, back[1] - 0.013) == 989 * 1400 + 559
        # the difference between the two results is the four texel values' doing and nothing else's
        sin_yaw = 1.0
        high = costmap_terms64(robust_track[1010, 560], robust_track[990, 560], p, 2.0, sin_yaw)
        low = costmap_terms64(robust_track[1009, 559], robust_track[989, 559], p, 2.0, sin_yaw)
        assert abs(float(got_literal) - high) <= 4 * np.spacing(np.float32(high)), (got_literal, high)
        assert abs(float(got_moved) - low) <= 4 * np.spacing(np.float32(low)), (got_moved, low)
        assert abs((float(got_literal) - float(got_moved)) - (high - low)) <= 8 * np.spacing(np.float32(high))


# ------------------------------------------------------------------ CPU: one hand-derived value per branch --------------
def hand_map(front, back):
    """3 rows x 5 columns of 1 m texels under bounds x in [0, 5], y in [0, 3]; a vehicle at (1, 1.5) with yaw 0 has its front
    point in texel (row 1, column 1) and its back point in (row 1, column 0).  Every other texel is poisoned with 99"""
    t = np.full((3, 5, 4), 99.0, np.float32)
    t[1, 1], t[1, 0] = front, back
    return t


def hand_params(**kw):
    p = m.ARRobustCostParams()
    p.setTransformFromBounds(0, 5, 0, 3)
    p.boundary_threshold, p.crash_coeff, p.track_coeff, p.track_slop = 0.5, 1000, 2, 0.3
    p.speed_coeff, p.heading_coeff, p.slip_coeff, p.desired_speed = 3, 0, 0, -1
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_costmap_branches_by_hand(host):
    """vehicle at (1, 1.5), yaw 0, vx = 4; front texel (boundary, track, speed, heading) and back texel given per case.
    threshold 0.5, crash_coeff 1000, track_coeff 2, track_slop 0.3, speed_coeff 3: every expected value is exact in float"""
    s = state(1, 1.5, vx=4)
    quiet_back = (0.2, 9, 9, 9)  # only .x of the back texel is read
    cases = [
        # front texel,            back,              parameters,                  expected
        ((0.4, 0.25, 5.0, 0.5), quiet_back, {}, 3.0),                             # constraint below the threshold, track off: 3 |4 - 5|
        ((0.75, 0.25, 5.0, 0.5), quiet_back, {}, 503.0),                          # on the ramp: (0.75 - 0.5) / 0.5 * 1000
        ((3.0, 0.25, 5.0, 0.5), quiet_back, {}, 1003.0),                          # saturated at 1: the whole crash_coeff
        ((0.4, 0.25, 5.0, 0.5), (0.75, 9, 9, 9), {}, 503.0),                      # the BACK texel's constraint decides
        ((0.4, 0.5, 5.0, 0.5), quiet_back, {}, 4.0),                              # track term on: 2 * 0.5
        ((0.4, 0.3, 5.0, 0.5), quiet_back, {}, 3.0),                              # at track_slop exactly: still off (>)
        ((0.4, 0.25, 5.0, 0.5), quiet_back, dict(desired_speed=6.0), 6.0),        # speed from desired_speed: 3 |4 - 6|
        ((0.4, 0.25, 5.0, 0.5), quiet_back, dict(heading_coeff=4.0), 5.0),        # heading: 4 |sin 0 + 0.5| on top of 3
        ((0.5, 0.25, 5.0, 0.5), quiet_back, {}, 3.0),                             # at the threshold exactly: on the ramp, alpha 0
    ]
    for front, back, kw, want in cases:
        host.set_costmap(hand_map(front, back))
        host.set_cost_params(hand_params(**kw))
        got = host.terms(s)
        assert got[0] == 0.0 and got[1] == np.float32(want), (front, back, kw, got, want)
        assert host.cost(s) == np.float32(want)
    # yaw pi/2: the front point is half a metre up the rows; sin = 1, heading 4 |1 + 0.5| = 6 on top of 3
    t = np.full((3, 5, 4), 99.0, np.float32)
    t[2, 1], t[1, 1] = (0.4, 0.25, 5.0, 0.5), (0.2, 9, 9, 9)
    host.set_costmap(t)
    host.set_cost_params(hand_params(heading_coeff=4.0))
    assert abs(host.terms(state(1.5, 1.9, yaw=np.pi / 2, vx=4))[1] - 9.0) <= 1e-6 * 9


def test_slip_and_roll_branches_by_hand(host):
    """slip_coeff 10, max_slip_ang 1, crash_coeff 1000, vx = 1, vy = tan(slip).  Below the ramp (slip 0.5): 10 slip.  On it
    (0.875): alpha = (0.875 - 0.75) / 0.25 = 0.5 -> 500 + 8.75.  Past max_slip_ang (1.2): 1000 + 12.  A roll of float(pi/2), which
    is above the double pi/2, REPLACES the ramp's penalty by crash_coeff: 1000 + 8.75, not 1500 + 8.75; the next float below is no
    roll.  |vx| < 0.001: slip 0 whatever vy is.  Bar: 1e-5 relative — det::atan's 3 ulp through the ramp's slope of 4000 is 1e-3
    absolute on 508.75."""
    host.set_costmap(hand_map((0, 0, 0, 0), (0, 0, 0, 0)))
    host.set_cost_params(hand_params(slip_coeff=10, max_slip_ang=1.0))
    half_pi = np.float32(np.pi / 2)
    for slip, roll, want in ((0.5, 0, 5.0), (0.875, 0, 508.75), (1.2, 0, 1012.0), (0.875, half_pi, 1008.75), (0.875, -half_pi, 1008.75),
                             (0.875, np.nextafter(half_pi, np.float32(0)), 508.75), (0.5, half_pi, 1005.0)):
        for sign in (1, -1):  # the slip is an absolute value, and so is vx's part in it
            got = float(host.stabilizing(state(vx=sign * 1.0, vy=np.tan(slip), roll=roll)))
            assert abs(got - want) <= 1e-5 * want, (slip, roll, sign, got, want)
            got = float(host.stabilizing(state(vx=1.0, vy=sign * np.tan(slip), roll=roll)))
            assert abs(got - want) <= 1e-5 * want, (slip, roll, sign, got, want)
    assert host.stabilizing(state(vx=0.0009, vy=5.0)) == 0.0 and host.stabilizing(state(vx=-0.0009, vy=5.0)) == 0.0
    assert abs(float(host.stabilizing(state(vx=0.0011, vy=5.0))) - (1000 + 10 * np.arctan(5 / 0.0011))) < 1e-2


def test_boundary_threshold_one_is_max_cost_and_nan_is_max_cost(host):
    """boundary_threshold == 1 with a constraint of 1 is (1 - 1) / (1.0 - 1) = 0 / 0: the step costs MAX_COST_VALUE — the
    reference's behaviour, kept.  A constraint below 1 at that threshold is no penalty.  A NaN state is MAX_COST_VALUE too"""
    s = state(1, 1.5, vx=4)
    host.set_cost_params(hand_params(boundary_threshold=1.0))
    host.set_costmap(hand_map((1.0, 0.25, 5.0, 0.5), (0.2, 9, 9, 9)))
    assert host.cost(s) == MAX_COST
    host.set_costmap(hand_map((7.0, 0.25, 5.0, 0.5), (0.2, 9, 9, 9)))  # clamped to 1 first
    assert host.cost(s) == MAX_COST
    host.set_costmap(hand_map((0.99, 0.25, 5.0, 0.5), (0.2, 9, 9, 9)))
    assert host.cost(s) == np.float32(3.0)
    host.set_cost_params(hand_params())
    for bad in (2, 4, 5):
        y = s.copy()
        y[bad] = np.nan
        assert host.cost(y) == MAX_COST, bad
    # a NaN position clamps to texel (0, 0) (NaN -> 0), it is no NaN cost
    t = hand_map((0.4, 0.25, 5.0, 0.5), (0.2, 9, 9, 9))
    t[0, 0] = (0.0, 0.0, 4.0, 0.0)
    host.set_costmap(t)
    assert host.cost(state(np.nan, np.nan, vx=4)) == 0.0


# ------------------------------------------------------------------ the small map of the GPU tests ----------------------
MAP_W, MAP_H = 28, 22
# 0.1 m texels around the start of common.autorally_cfg, (-12, 5); in float32, (max - min) * 10 truncates to 28 and 22, which is
# how the reference's loader sizes a map (test_npz_loader_interleaves_four_channels)
MAP_BOUNDS = (-12.5, -9.7, 3.8, 6.0)


def small_map():
    """22 rows x 28 columns (width != height).  Channel 0 in bands of 0 / 0.6 / 1 by column (three columns earlier from row 16
    on), channel 1 on both sides of track_slop = 1.0, channels 2 and 3 varying with row and column"""
    r, c = np.meshgrid(np.arange(MAP_H), np.arange(MAP_W), indexing="ij")
    band = c + 3 * (r >= 16)
    c0 = np.where(band >= 20, 1.0, np.where(band >= 16, 0.6, 0.0))
    return ar.interleave([c0, 0.05 * c + 0.01 * r, 3.0 + 0.1 * c - 0.05 * r, 0.3 - 0.02 * c + 0.01 * r])


def robust_cfg(K=65, T=3, D=1, second=False, num_iters=1):
    """common.autorally_cfg's synthetic network and sampler, with ARRobustCost on small_map(), dt = 0.1.  The vehicle starts at
    (-12.05, 5.05) at 4 m/s along +x and covers four columns a step: its footprint's constraint is 0 on step 1, 0.6 (the ramp from
    boundary_threshold = 0.5) on step 2 and 1 from step 3 on; the front texel's channel 1 crosses track_slop between steps 2 and
    3; from step 5 on its front point is beyond the map (clamped).  vy starts at -0.05 and the network pushes it further: the slip crosses
    0.75 max_slip_ang = 0.0225 on step 2 and max_slip_ang = 0.03 on step 3, with the rollouts on both sides.
    second: the roll starts at 1.55 and passes pi/2 on the first step, boundary_threshold = 1 (MAX_COST_VALUE wherever the
    constraint is 1), and the speed target is desired_speed"""
    base = autorally_cfg(K=K, T=T, num_iters=num_iters)
    cost = m.ARRobustCostParams()
    cost.setTransformFromBounds(*MAP_BOUNDS)
    cost.boundary_threshold, cost.track_slop, cost.heading_coeff, cost.slip_coeff = 0.5, 1.0, 20, 10
    cost.crash_coeff, cost.max_slip_ang = 10000, 0.03
    x0 = np.array([-12.05, 5.05, 0.0, 0.0, 4.0, -0.05, 0.0], np.float32)
    if second:
        cost.boundary_threshold, cost.desired_speed = 1.0, 5.0
        x0[3] = 1.55
    return dict(base, model="autorally_nn_robust", D=D, dt=0.1, cost=cost, x0=x0,
                blobs={"dynamics_weights": base["blobs"]["dynamics_weights"], "costmap": small_map()})


def make_robust_oracle(cfg):
    o = ar.ARRobustOracle(cfg["K"], cfg["T"], cfg["D"], cfg["dt"], cfg["lambda_"], cfg["alpha"], cfg["num_iters"])
    o.set_cost_params(cfg["cost"])
    for name, arr in cfg["blobs"].items():
        o.set_blob(name, arr)
    o.set_control_ranges(cfg["ranges"])
    o.set_sampler(cfg["std_dev"], cfg["control_cost_coeff"], cfg.get("pure_pct", 0.01), cfg.get("decay", 1.0))
    return o


# ------------------------------------------------------------------ CPU: shipped class == restatement, bit for bit -------
def scattered_states(n, seed, cfg):
    """states over and beyond small_map(): positions up to 1 m outside the bounds, any yaw, speeds on both sides of 0.001,
    slips on both sides of the ramp (max_slip_ang is set to 0.6 for these), rolls on both sides of pi/2"""
    rng = np.random.default_rng(seed)
    x0b, x1b, y0b, y1b = MAP_BOUNDS
    s = np.zeros((n, 7))
    s[:, 0] = rng.uniform(x0b - 1, x1b + 1, n)
    s[:, 1] = rng.uniform(y0b - 1, y1b + 1, n)
    s[:, 2] = rng.uniform(-4, 4, n)
    s[:, 3] = rng.choice([0.0, 0.3, 1.5, 1.6, -1.7], n) + rng.uniform(-0.05, 0.05, n)
    s[:, 4] = rng.choice([4.0, 1.0, -2.0, 0.0005], n) * rng.uniform(0.5, 1.5, n)
    s[:, 5] = rng.uniform(-1.5, 1.5, n) * np.abs(s[:, 4])
    s[:, 6] = rng.uniform(-1, 1, n)
    return s.astype(np.float32)


def test_shipped_class_equals_restatement_bitwise(host):
    cfg = robust_cfg()
    o = make_robust_oracle(cfg)
    host.set_costmap(small_map())
    p = cfg["cost"]
    p.max_slip_ang = 0.6
    for desired_speed, threshold in ((-1, 0.5), (5.0, 0.5), (-1, 1.0), (-1, 0.0)):
        p.desired_speed, p.boundary_threshold = desired_speed, threshold
        host.set_cost_params(p)
        o.set_cost_params(p)
        xs = np.concatenate([scattered_states(500, 11, cfg), [state(np.nan, 5, vx=4), state(-11, 5, vx=np.nan), state(-11, 5, np.inf, vx=4)]])
        n_max = 0
        for i, x in enumerate(xs):
            a, b = host.terms(x), o.terms(x)
            assert bits_equal(a, b[[0, 5]], nan_equal=True), (i, x, a, b)
            ca, cb = host.cost(x, i), o.cost(x, i)
            assert bits(ca) == bits(cb), (i, x, ca, cb)
            n_max += ca == MAX_COST
        assert n_max >= 2, n_max  # the two NaN states at least
        if threshold == 1.0:
            assert n_max > 20, n_max  # and every state whose constraint is 1


# ------------------------------------------------------------------ CPU: restatement against float64 --------------------
def cost64(s, p, texels):
    """(total, sum of the terms' magnitudes, smallest distance of a compared quantity to its threshold or texel boundary) in
    float64 numpy; shares nothing with the C++"""
    s = np.asarray(s, np.float64)
    h, w = texels.shape[:2]
    r1, r2, tr = (np.asarray(a[:], np.float64) for a in (p.r_c1, p.r_c2, p.trs))
    gaps, terms = [], []
    slip = 0.0 if abs(s[4]) < 0.001 else abs(np.arctan(s[5] / abs(s[4])))
    gaps += [abs(abs(s[4]) - 0.001), abs(slip - 0.75 * p.max_slip_ang), abs(abs(s[3]) - np.pi / 2)]
    penalty = 0.0
    if slip >= 0.75 * p.max_slip_ang:
        penalty = (min(1.0, slip / p.max_slip_ang) - 0.75) / 0.25 * p.crash_coeff
    if abs(s[3]) >= np.pi / 2:
        penalty = p.crash_coeff
    terms += [p.slip_coeff * slip, penalty]
    found = []
    for d in (0.5, -0.5):
        pos = np.array([s[0] + d * np.cos(s[2]), s[1] + d * np.sin(s[2]), 1.0])
        uvw = r1 * pos[0] + r2 * pos[1] + tr
        fu, fv = uvw[0] / uvw[2] * w, uvw[1] / uvw[2] * h
        gaps += [abs(fu - np.round(fu)), abs(fv - np.round(fv))]
        found.append(texels[int(np.clip(np.floor(fv), 0, h - 1)), int(np.clip(np.floor(fu), 0, w - 1))].astype(np.float64))
    front, back = found
    c = min(1.0, max(front[0], back[0]))
    gaps += [abs(c - p.boundary_threshold), abs(front[1] - p.track_slop)]
    terms.append((c - p.boundary_threshold) / (1.0 - p.boundary_threshold) * p.crash_coeff if c >= p.boundary_threshold else 0.0)
    terms.append(p.track_coeff * front[1] if front[1] > p.track_slop else 0.0)
    terms.append(p.speed_coeff * abs(s[4] - (front[2] if p.desired_speed == -1 else p.desired_speed)))
    terms.append(p.heading_coeff * abs(np.sin(s[2]) + front[3]))
    return float(np.sum(terms)), float(np.sum(np.abs(terms))), float(min(gaps))


def test_restatement_against_float64():
    """The CPU restatement against the independent float64 one on small_map(), 1e-4 relative of the sum of the terms' magnitudes.
    The cost jumps at its thresholds and at texel boundaries, so the states are DRAWN at least MARGIN = 1e-3 from every one of
    them — |vx| against 0.001, the slip against 0.75 max_slip_ang, |roll| against pi/2, both query points' texture coordinates
    (in texels) against the next integer, the constraint against boundary_threshold, the track value against track_slop: the draw
    (float64 side only) replaces a candidate that is closer.  Every state drawn is compared and the margin is asserted again"""
    cfg = robust_cfg()
    p = cfg["cost"]
    p.max_slip_ang, p.boundary_threshold = 0.6, 0.45
    texels = small_map()
    o = make_robust_oracle(cfg)
    worst, taken = 0.0, np.zeros(6, int)
    for desired_speed in (-1, 5.0):
        p.desired_speed = desired_speed
        o.set_cost_params(p)
        drawn, seed = [], 30
        while len(drawn) < 400:
            for x in scattered_states(200, seed, cfg):
                if cost64(x, p, texels)[2] >= MARGIN and len(drawn) < 400:
                    drawn.append(x)
            seed += 1
        for x in drawn:
            want, scale, gap = cost64(x, p, texels)
            assert gap >= MARGIN
            got = float(o.cost(x))
            worst = max(worst, abs(got - want) / scale)
            t = o.terms(x)
            taken += [t[1] == 0, 0 < t[1] < p.crash_coeff, t[1] == p.crash_coeff, t[2] > 0, t[0] > p.crash_coeff / 2, abs(x[3]) > np.pi / 2]
    print("cost against float64: %.3g relative; branches taken %s" % (worst, taken))
    assert (taken > 0).all(), taken
    assert worst <= REL_TOL, worst


# ------------------------------------------------------------------ CPU: parameter block, blob rules, registration ------
def test_parameter_block_layout_in_c_cpp_and_python(host):
    """size and the offset of every field agree between model_params.h, the plugin's class and the Python mirror; the class's
    defaults, copied out of C++, are the mirror's defaults byte for byte; the block is the standard one plus heading_coeff"""
    in_class, in_pod = np.zeros(16, np.int32), np.zeros(16, np.int32)
    assert host.L.robust_cost_field_offsets(in_class, in_pod) == 15
    names = [f[0] for f in m.ARRobustCostParams._fields_]
    mirror = [getattr(m.ARRobustCostParams, n).offset for n in names] + [C.sizeof(m.ARRobustCostParams)]
    assert len(names) == 15 and in_class.tolist() == in_pod.tolist() == mirror
    assert mirror[-1] == C.sizeof(m.ARStandardCostParams) + 4 == 4 * 22
    assert names[:-1] == [f[0] for f in m.ARStandardCostParams._fields_] and names[-1] == "heading_coeff"
    block = m.ARRobustCostParams()
    block.crash_coeff = -1
    host.L.robust_cost_default_params(C.byref(block))
    d = m.ARRobustCostParams()
    assert bytes(block) == bytes(d)
    assert list(d.control_cost_coeff) == [0, 0] and d.discount == 1.0
    assert (d.desired_speed, d.max_slip_ang, d.track_coeff, d.slip_coeff, d.speed_coeff) == (-1, 1.5, 33, 0, 20)
    assert (d.crash_coeff, d.boundary_threshold, d.track_slop, d.heading_coeff, d.grid_res) == (125000, 0.75, 0, 0, 10)
    d.setTransformFromBounds(-25, 45, -50, 5)
    s = m.ARStandardCostParams()
    s.setTransformFromBounds(-25, 45, -50, 5)
    assert (list(d.r_c1), list(d.r_c2), list(d.trs)) == (list(s.r_c1), list(s.r_c2), list(s.trs))


def test_registration_equals_autorally_nn(robust_model):
    assert m.list_models().count("autorally_nn_robust") == 1
    ar.load_model(m)  # a second load is a no-op
    assert m.list_models().count("autorally_nn_robust") == 1
    d, a = m.describe_model("autorally_nn_robust"), m.describe_model("autorally_nn")
    assert d["rmppi"] and d["rmppi_pipeline"] and (8, 16, 1) in d["shapes"] and (64, 4, 2) in d["replicated_lane_shapes"]
    assert {k: v for k, v in d.items() if k != "name"} == {k: v for k, v in a.items() if k != "name"}
    assert m.describe_model("autorally_nn_robust", m.MPPI_SAMPLER_COLORED) is None


def test_unregister_and_reload(robust_model):
    """mppi_unregister_model: an unknown name is MPPI_ERR_UNKNOWN_MODEL; a registered one leaves the listing and mppi_describe_model;
    a second unregister is MPPI_ERR_UNKNOWN_MODEL again; loading the plugin library again (its static initialisers do not run a
    second time) puts the registration back, once"""
    lib_ = robust_model
    G = m.MPPI_SAMPLER_GAUSSIAN
    assert lib_.mppi_unregister_model(b"no_such_model", G) == m.MPPI_ERR_UNKNOWN_MODEL
    assert lib_.mppi_unregister_model(b"autorally_nn_robust", m.MPPI_SAMPLER_COLORED) == m.MPPI_ERR_UNKNOWN_MODEL
    assert lib_.mppi_unregister_model(None, G) == m.MPPI_ERR_INVALID_ARG
    before = m.describe_model("autorally_nn_robust")
    try:
        assert lib_.mppi_unregister_model(b"autorally_nn_robust", G) == m.MPPI_OK
        assert "autorally_nn_robust" not in m.list_models() and m.describe_model("autorally_nn_robust") is None
        assert "autorally_nn" in m.list_models()
        assert lib_.mppi_unregister_model(b"autorally_nn_robust", G) == m.MPPI_ERR_UNKNOWN_MODEL
    finally:
        ar.load_model(m)
    assert m.list_models().count("autorally_nn_robust") == 1 and m.describe_model("autorally_nn_robust") == before


# ------------------------------------------------------------------ GPU: the branch census, first ------------------------
SHAPES = [(1, 1), (65, 3), (200, 5), (1049, 9)]  # injected noise; (65, 17) runs with Philox
_REFERENCE = {}


def _reference_run(K, T, second=False):
    """two consecutive Vanilla calls of the CPU restatement with a slide between, computed once per (K, T, configuration) and
    shared read-only"""
    key = (K, T, second)
    if key not in _REFERENCE:
        cfg = robust_cfg(K=K, T=T, second=second)
        o = make_robust_oracle(cfg)
        x1 = o.model_step(cfg["x0"], np.zeros(2, np.float32))[0]
        calls = []
        for i, x in enumerate((cfg["x0"], x1)):
            eps = host_noise(1, K, T, 2, seed=K + T + i)
            mean = o.control().copy()
            o.vanilla_compute_control(x, 1, eps)
            calls.append(dict(x=x, eps=eps, mean=mean, costs=o.costs().copy(), control=o.control().copy(), samples=o.samples().copy()))
            o.vanilla_slide(1)
        for c in calls:
            for a in c.values():
                a.setflags(write=False)
        _REFERENCE[key] = calls
    return _REFERENCE[key]


FIRST = ("below_threshold", "on_ramp", "saturated", "track_on", "track_off", "speed_from_map", "heading", "slip_below", "slip_ramp",
         "slip_saturated")
SECOND = ("rolled", "max_cost", "speed_from_param")


def test_gpu_inputs_take_every_branch():
    """what the GPU comparison is worth, counted on the restatement over the rollout-steps of the first call: at every shape with
    T >= 3 — (65, 3), (200, 5), (1049, 9), (65, 17) — at least one rollout-step has the constraint below the threshold, one on
    the ramp and one saturated; the track term on and off; the speed taken from the map; a non-zero heading term; the slip below
    its ramp, on it and saturated.  The second configuration adds, at the same shapes, the roll branch, MAX_COST_VALUE and the
    speed from desired_speed.  (1, 1) is one rollout-step: it can take one branch of each kind, and is asserted to be counted
    once in each."""
    for K, T in SHAPES + [(65, 17)]:
        for second, wanted in ((False, FIRST), (True, SECOND)):
            cfg = robust_cfg(K=K, T=T, second=second)
            o = make_robust_oracle(cfg)
            if (K, T) == (65, 17):
                o.set_nominal_control(np.zeros((T, 2), np.float32))
                o.vanilla_compute_control(cfg["x0"], 1, po.philox_normal(PHILOX_SEED, 0, K, T, 2)[None])
                samples = o.samples()[0]
            else:
                samples = _reference_run(K, T, second)[0]["samples"][0]
            counts = o.census(cfg["x0"], samples)
            print("K=%d T=%d%s: %s" % (K, T, " second" if second else "", counts))
            n = K * T
            assert counts["below_threshold"] + counts["on_ramp"] + counts["saturated"] == n
            assert counts["track_on"] + counts["track_off"] == n and counts["speed_from_map"] + counts["speed_from_param"] == n
            assert counts["slip_below"] + counts["slip_ramp"] + counts["slip_saturated"] == n
            if T >= 3:
                assert all(counts[k] > 0 for k in wanted), (K, T, second, counts)


# ------------------------------------------------------------------ GPU: every form of the registration -----------------
def _cases(controller):
    from kernel_forms import build_cases
    return [c for c in build_cases() if c["model"] == "autorally_nn_robust" and c["controller"] == controller]


VANILLA_FORMS = ["fused64x4x1", "pipeline64x4x1", "fused32x4x1", "fused8x16x1", "fused16x8x1", "fused16x4x1", "fused64x1x1",
                 "fused64x4x1-hbm", "pipeline64x4x1-hbm"]
TUBE_FORMS = ["fused64x4x2", "fused32x4x2", "fused8x16x2", "fused64x4x2-hbm"]
ROBUST_FORMS = ["fused64x1x2", "fused32x1x2", "pipeline64x1x2"]


def _form(case):
    return case["id"].split("-", 2)[2]


def test_forms_follow_kernel_forms(robust_model):
    """the lists the GPU tests are parametrised over are what kernel_forms.build_cases() enumerates from mppi_describe_model and
    pipeline_family for this registration: the fused LDS shapes, the MFMA replicated-lane shapes fused and role-pipelined, rows
    in HBM; both BZ = 2 families for Tube; the Robust kernels"""
    from kernel_forms import pipeline_family
    d = m.describe_model("autorally_nn_robust")
    assert pipeline_family(d, (64, 4, 1)) == "pipeline_rep" and pipeline_family(d, (8, 16, 1)) is None
    for ctl, forms in (("vanilla", VANILLA_FORMS), ("tube", TUBE_FORMS), ("robust", ROBUST_FORMS)):
        got = [_form(c) for c in _cases(ctl) if not c["refuse"]]
        assert got == forms, (ctl, got)
    families = {c["expect"]["family"] for ctl in ("vanilla", "tube", "robust") for c in _cases(ctl) if not c["refuse"]}
    assert families == {"fused", "fused_rep", "pipeline_rep", "rmppi", "rmppi_pipeline"}


def _case(controller, form):
    (case,) = [c for c in _cases(controller) if _form(c) == form]
    return case


def _engine(case, cfg, **extra):
    from kernel_forms import env_override
    env = {"MPPI_AMD_ROWS_IN_HBM": "1" if case["hbm"] else "0"}
    with env_override(**env):
        return make_engine(cfg, save_samples=True, **dict(case["kw"], **extra))


_FIRST_FORM_COSTS = {}


def _first_form_costs(K, T, second):
    """the costs of both calls on VANILLA_FORMS[0], run here when no test has run that form at this shape yet: whichever form is
    selected, alone or in any order, it is compared with the first one"""
    key = (K, T, second)
    if key not in _FIRST_FORM_COSTS:
        eng = _engine(_case("vanilla", VANILLA_FORMS[0]), robust_cfg(K=K, T=T, second=second))
        try:
            out = []
            for c in _reference_run(K, T, second):
                eng.updateImportanceSampler(c["mean"])
                eng.injectNoise(c["eps"])
                eng.computeControl(c["x"], 1)
                out.append(eng.getSampledCostSeq().copy())
                eng.slideControlSequence(1)
            _FIRST_FORM_COSTS[key] = out
        finally:
            eng.close()
    return _FIRST_FORM_COSTS[key]


@pytest.mark.gpu
@pytest.mark.parametrize("form", VANILLA_FORMS)
def test_every_vanilla_form_against_restatement(gpu, robust_model, form):
    """(K, T) = (1, 1), (65, 3), (200, 5), (1049, 9) with injected noise, both configurations at (200, 5), two calls with a slide
    between: trajectory costs 0 ulp, clamped samples 0 ulp, u* within 1e-5, and every form's costs equal the first form's bit
    for bit; then (65, 17) with the in-kernel Philox stream, two calls with a slide between, to the same bars"""
    from kernel_forms import check_form
    case = _case("vanilla", form)
    for K, T, second in [(K, T, False) for K, T in SHAPES] + [(200, 5, True)]:
        cfg = robust_cfg(K=K, T=T, second=second)
        eng = _engine(case, cfg)
        try:
            for i, c in enumerate(_reference_run(K, T, second)):
                tag = "%s K=%d T=%d%s call %d" % (form, K, T, " second" if second else "", i)
                if i > 0:
                    assert np.abs(eng.getControlSeq() - c["mean"]).max() <= U_TOL, tag
                eng.updateImportanceSampler(c["mean"])
                eng.injectNoise(c["eps"])
                eng.computeControl(c["x"], 1)
                check_form(case, eng, tag)
                costs = eng.getSampledCostSeq()
                dc = int(ulp_diff(costs, c["costs"]).max())
                dv = int(ulp_diff(eng.getSampledControls(), c["samples"]).max())
                du = float(np.abs(eng.getControlSeq() - c["control"]).max())
                print("%s: costs %d ulp, samples %d ulp, u* %.3g" % (tag, dc, dv, du))
                assert dc == 0, "%s: costs differ by up to %d ulp" % (tag, dc)
                assert dv == 0, "%s: clamped samples differ by up to %d ulp" % (tag, dv)
                assert du <= U_TOL, "%s: u* differs by %g" % (tag, du)
                assert np.array_equal(bits(costs), bits(_first_form_costs(K, T, second)[i])), tag
                eng.slideControlSequence(1)
        finally:
            eng.close()
    K, T = 65, 17
    cfg = robust_cfg(K=K, T=T)
    eng = _engine(case, cfg)
    try:
        eng.setSeed(PHILOX_SEED)
        o = make_robust_oracle(cfg)
        x = cfg["x0"]
        for call in range(2):  # the second launch draws generation 1 of the same stream
            if call > 0:
                assert np.abs(eng.getControlSeq() - o.control()).max() <= U_TOL
                eng.updateImportanceSampler(o.control())  # both sides start from the same slid mean
                x = o.model_step(x, np.zeros(2, np.float32))[0]
            eng.computeControl(x, 1)
            check_form(case, eng, form + " philox")
            o.vanilla_compute_control(x, 1, po.philox_normal(PHILOX_SEED, call, K, T, 2)[None])
            dc = int(ulp_diff(eng.getSampledCostSeq(), o.costs()).max())
            dv = int(ulp_diff(eng.getSampledControls(), o.samples()).max())
            du = float(np.abs(eng.getControlSeq() - o.control()).max())
            print("%s philox K=65 T=17 call %d: costs %d ulp, samples %d ulp, u* %.3g" % (form, call, dc, dv, du))
            assert dc == 0 and dv == 0 and du <= U_TOL, (form, call, dc, dv, du)
            eng.slideControlSequence(1)
            o.vanilla_slide(1)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", TUBE_FORMS)
def test_tube_forms_against_restatement(gpu, robust_model, form):
    """Tube MPPI on the two-system shapes, both families (the LDS form (8, 16, 2), the MFMA replicated-lane forms (64, 4, 2) and
    (32, 4, 2)) and rows in HBM, at (65, 3) and (200, 5): trajectory costs of both systems 0 ulp, clamped samples 0 ulp, u* and the
    nominal u* within 1e-5; the second configuration (roll, MAX_COST_VALUE, desired_speed) at (200, 5) too"""
    from kernel_forms import check_against_oracle, check_form, compute_once
    case = _case("tube", form)
    for K, T, second in ((65, 3, False), (200, 5, False), (200, 5, True)):
        cfg = robust_cfg(K=K, T=T, D=2, second=second)
        eng, orc = _engine(case, cfg), make_robust_oracle(cfg)
        try:
            tag = "tube %s K=%d T=%d%s" % (form, K, T, " second" if second else "")
            compute_once(case, [eng], orc, None, cfg, 1, host_noise(1, K, T, 2, seed=K + T), False, None)
            check_form(case, eng, tag)
            du = check_against_oracle(case, eng, orc, tag, samples_exact=True, show=True)
            assert du <= U_TOL, "%s: u* (or the nominal u*) differs by %g" % (tag, du)
        finally:
            eng.close()


def _robust_pair(case, cfg, K):
    nc, ns = (9, 32) if K >= 9 * 32 else (3, K // 3)
    eng = m.RobustMPPIController(cfg["model"], cfg["K"], cfg["T"], cfg["dt"], cfg["lambda_"], cfg["alpha"], cfg["num_iters"],
                                 seed=SEED, save_samples=True, **case["kw"])
    eng.setCostParams(cfg["cost"])
    for name, blob in cfg["blobs"].items():
        eng.setModelBlob(name, blob)
    eng.setControlRanges(cfg["ranges"])
    eng.setSamplingParams(cfg["std_dev"], cfg["control_cost_coeff"], 0.01, 1.0)
    eng.setRMPPIParams(1000.0, nc, ns)
    orc = make_robust_oracle(cfg)
    return eng, orc, po.RobustOracle(orc, 1000.0, nc, ns)


@pytest.mark.gpu
@pytest.mark.parametrize("reduction", ["default", "reference-order"])
@pytest.mark.parametrize("form", ROBUST_FORMS)
def test_robust_forms_against_restatement(gpu, robust_model, form, reduction):
    """Robust MPPI at (65, 3) and (200, 5) with the feedback gains set, control cost coefficients (0.2, 0.1).  First cycle (no
    candidates yet): the nominal / real kernel — costs of both systems 0 ulp, u* and nominal u* within 1e-5.  In reference-order
    reduction the handle is the restatement bit for bit, so a second cycle follows from the state the first one's control leads
    to: the init-eval kernel scores the candidates (best candidate, nominal state and the candidates' free energies equal the
    restatement's bits), then the nominal / real kernel again — costs 0 ulp, u* and nominal u* the same bits.  The second
    configuration runs at (200, 5) too.  The default-reduction handle stops after the first cycle: its u* is within 1e-5 of the
    restatement's and not its bits, the candidates of a second cycle are scored from that u*, and no call sets a Robust handle's
    nominal control, so nothing exact could be asserted of them.  The reduction mode changes the last stage of an iteration only:
    the init-eval and rollout kernels the reference-order handle runs are the ones the default handle runs"""
    from kernel_forms import check_against_oracle, check_form, compute_once
    case = _case("robust", form)
    exact = reduction == "reference-order"
    for K, T, second in ((65, 3, False), (200, 5, False), (200, 5, True)):
        cfg = robust_cfg(K=K, T=T, D=2, second=second)
        cfg["control_cost_coeff"] = [0.2, 0.1]
        eng, orc, rob = _robust_pair(case, cfg, K)
        try:
            if exact:
                eng.setReductionMode(m.MPPI_REDUCTION_REFERENCE_ORDER)
            tag = "robust %s %s K=%d T=%d%s" % (form, reduction, K, T, " second" if second else "")
            noise = host_noise(1, K, T, 2, seed=K + T)
            compute_once(case, [eng], orc, rob, cfg, 1, noise, False, None)
            check_form(case, eng, tag)
            du = check_against_oracle(case, eng, orc, tag, show=True)
            assert du <= U_TOL, "%s: u* (or the nominal u*) differs by %g" % (tag, du)
            if not exact:
                continue
            assert bits_equal(eng.getControlSeq(), orc.control()) and bits_equal(eng.getNominalControlSeq(), orc.nominal_control()), tag
            x1 = orc.model_step(cfg["x0"], orc.control()[0])[0]
            noise = host_noise(1, K, T, 2, seed=K + T + 1)
            compute_once(case, [eng], orc, rob, dict(cfg, x0=x1), 1, noise, False, None, candidate_noise=noise[0], first_cycle=False)
            ns_e, best_e, stride_e, fe_e = eng.getRMPPIState()
            ns_o, best_o, stride_o, fe_o = rob.state()
            assert (best_e, stride_e) == (best_o, stride_o), (tag, best_e, stride_e, best_o, stride_o)
            assert bits_equal(ns_e, ns_o, nan_equal=True) and bits_equal(fe_e, fe_o, nan_equal=True), (tag, fe_e, fe_o)
            du = check_against_oracle(case, eng, orc, tag + " cycle 2", show=True)
            assert bits_equal(eng.getControlSeq(), orc.control()) and bits_equal(eng.getNominalControlSeq(), orc.nominal_control()), tag
        finally:
            eng.close()


@pytest.mark.gpu
def test_handle_outlives_unregistering(gpu, robust_model):
    """a handle created before mppi_unregister_model owns its model object and still computes the restatement's costs; no new
    handle can be created until the plugin is loaded again"""
    K, T = 200, 5
    cfg, want = robust_cfg(K=K, T=T), _reference_run(K, T)[0]
    eng = make_engine(cfg, save_samples=True)
    try:
        assert robust_model.mppi_unregister_model(b"autorally_nn_robust", m.MPPI_SAMPLER_GAUSSIAN) == m.MPPI_OK
        try:
            eng.updateImportanceSampler(want["mean"])
            eng.injectNoise(want["eps"])
            eng.computeControl(want["x"], 1)
            assert int(ulp_diff(eng.getSampledCostSeq(), want["costs"]).max()) == 0
            with pytest.raises(m.MPPIError) as e:
                make_engine(cfg)
            assert e.value.status == m.MPPI_ERR_UNKNOWN_MODEL
        finally:
            ar.load_model(m)
        make_engine(cfg).close()
    finally:
        eng.close()


# ------------------------------------------------------------------ GPU: the loader and the blob's rules ----------------
def _refused(eng, name, array, count=None, dims=None):
    a = np.ascontiguousarray(array, np.float32)
    dims = a.shape if dims is None else dims
    st = eng._lib.mppi_set_model_blob(eng._h, name.encode(), a.reshape(-1), a.size if count is None else count,
                                      (C.c_int * len(dims))(*dims), len(dims))
    return st, (eng._lib.mppi_last_error(eng._h) or b"").decode()


# What the "costmap" blob and the loader accept and refuse is a property of a handle's model object, and mppi_create gives no handle
# without a HIP device (MPPI_ERR_NO_DEVICE; the library has no CPU path): these checks cannot run without one.  What needs no
# device — the channel count a class declares, the parameter block — is in the CPU tests above.
WANT_4 = ("costmap: this model's cost reads 4 channels: dims must be {height, width, 4} (interleaved texels) with "
          "height*width*4 == count")
WANT_1 = "costmap: dims must be {height, width} with height*width == count"


@pytest.mark.gpu
def test_npz_loader_interleaves_four_channels(gpu, robust_model, tmp_path):
    """mppi_load_npz("costmap") on an archive with channel0 .. channel3 in the reference's layout (flat, width = x extent *
    pixelsPerMeter) gives the costs of the "costmap" blob + setTransformFromBounds; an archive without channel3 is refused; the
    same four-channel archive loads into "autorally_nn" as channel0 alone, as before"""
    K, T = 200, 5
    cfg = robust_cfg(K=K, T=T)
    want = _reference_run(K, T)[0]
    texels = small_map()
    x0b, x1b, y0b, y1b = MAP_BOUNDS
    arrays = dict(xBounds=np.array([x0b, x1b], np.float32), yBounds=np.array([y0b, y1b], np.float32),
                  pixelsPerMeter=np.array([10.0], np.float32))
    for c in range(4):
        arrays["channel%d" % c] = texels[:, :, c].reshape(-1)
    assert int((arrays["xBounds"][1] - arrays["xBounds"][0]) * arrays["pixelsPerMeter"][0]) == MAP_W
    assert int((arrays["yBounds"][1] - arrays["yBounds"][0]) * arrays["pixelsPerMeter"][0]) == MAP_H
    path = tmp_path / "robust_map.npz"
    np.savez(path, **arrays)
    bare = dict(cfg, blobs={"dynamics_weights": cfg["blobs"]["dynamics_weights"]}, cost=m.ARRobustCostParams())
    for k in ("boundary_threshold", "track_slop", "heading_coeff", "slip_coeff", "crash_coeff", "max_slip_ang"):
        setattr(bare["cost"], k, getattr(cfg["cost"], k))  # everything but the transform: the loader installs that
    eng = make_engine(bare, save_samples=True)
    try:
        eng.loadNpz("costmap", path)
        eng.updateImportanceSampler(want["mean"])
        eng.injectNoise(want["eps"])
        eng.computeControl(want["x"], 1)
        assert int(ulp_diff(eng.getSampledCostSeq(), want["costs"]).max()) == 0
        assert np.abs(eng.getControlSeq() - want["control"]).max() <= U_TOL
        short = tmp_path / "three_channels.npz"
        np.savez(short, **{k: v for k, v in arrays.items() if k != "channel3"})
        with pytest.raises(m.MPPIError) as e:
            eng.loadNpz("costmap", short)
        assert e.value.status == m.MPPI_ERR_INVALID_ARG and "no key 'channel3'" in str(e.value), str(e.value)
    finally:
        eng.close()
    std = make_engine(autorally_cfg(K=64, T=4))
    try:
        std.loadNpz("costmap", path)  # channel0 alone, {height, width}
        std.computeControl(autorally_cfg()["x0"], 1)
    finally:
        std.close()


@pytest.mark.gpu
def test_costmap_blob_refusals(gpu, robust_model):
    """a {height, width} blob is refused on the four-channel model and a {height, width, 4} blob on "autorally_nn", each with a
    message that says what the model wants; wrong counts and channel numbers are refused too; the refused handle keeps its map"""
    cfg = robust_cfg(K=64, T=4)
    eng = make_engine(cfg)
    try:
        for kw in (dict(array=np.zeros((22, 28))), dict(array=np.zeros((22, 28, 1))), dict(array=np.zeros((22, 28, 3))),
                   dict(array=np.zeros((22, 28, 4)), count=22 * 28 * 4 - 1), dict(array=np.zeros((22, 28, 4)), dims=(22, 0, 4)),
                   dict(array=np.zeros(22 * 28 * 4))):
            st, msg = _refused(eng, "costmap", **kw)
            assert st == m.MPPI_ERR_INVALID_ARG and msg.endswith(WANT_4), (kw, st, msg)
        eng.computeControl(cfg["x0"], 1)
    finally:
        eng.close()
    std_cfg = autorally_cfg(K=64, T=4)
    std = make_engine(std_cfg)
    try:
        for arr in (np.zeros((22, 28, 4)), np.zeros((22, 28, 1))):
            st, msg = _refused(std, "costmap", arr)
            assert st == m.MPPI_ERR_INVALID_ARG and msg.endswith(WANT_1), (st, msg)
        std.computeControl(std_cfg["x0"], 1)
    finally:
        std.close()
