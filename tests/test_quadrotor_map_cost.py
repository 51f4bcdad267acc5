"""QuadrotorMapCost (the gate-racing cost over a track map) and its model, registered as "quadrotor_map".

CPU: the shipped class built for the host (tests/quadrotor_map_oracle/map_cost_host.hip) against hand-derived answers, one per
branch, and against the CPU restatement (tests/quadrotor_map_oracle/quadrotor_map_oracle.cpp) bit for bit; the restatement
against an independent float64 numpy restatement; the parameter block's layout in C, C++ and Python; updateWaypoint; the
registration.
GPU: every registered kernel form against the restatement (costs 0 ulp, clamped samples 0 ulp, u* within 1e-5) on inputs that
take every branch of the cost, with and without a map, with the waypoint moved between two calls; what the blobs refuse.
"""
import ctypes as C

import numpy as np
import pytest

import mppi_generic_amd as m
import pyoracle as po
import quadrotor_map_oracle as qm
from common import PHILOX_SEED, SEED, U_TOL, host_noise, make_engine, ulp_diff
from restate64 import bits
from test_quadrotor import euler64, quat_from_rpy64, random_states, rotation64

REL_TOL = 1e-4  # the quadrotor tests' bar against float64 (the reference's own rollout tolerance)
MARGIN = 1e-3   # every state compared with float64 is at least this far from every branch threshold (test_restatement_against_float64)
MAX_COST = np.float32(1e16)
LEVEL = [1.0, 0.0, 0.0, 0.0]


@pytest.fixture(scope="module")
def quadrotor_map(lib):
    """the registration unit is examples/quadrotor_model/quadrotor_map_model.hip: built on its own and loaded with
    mppi_load_plugin at test time, as tests/test_quadrotor.py does with "quadrotor" """
    return qm.load_model(m)


@pytest.fixture(scope="module")
def host():
    return qm.HostCost()


def state(pos, vel=(0, 0, 0), quat=LEVEL, rates=(0, 0, 0)):
    return np.concatenate([pos, vel, quat, rates]).astype(np.float32)


# ------------------------------------------------------------------ the track map of the tests --------------------------
def track_map():
    """9 rows x 7 columns (not square, both odd): a valley along the middle column that rises to 4.2 at the left and right
    edges, tilted a little along the rows — values on both sides of track_slop = 0.6 and of track_boundary_cost = 2.5"""
    r, c = np.meshgrid(np.arange(9), np.arange(7), indexing="ij")
    return (1.4 * np.abs(c - 3) + 0.05 * r).astype(np.float32)


def track_frame():
    """the map's frame: origin off the world's, turned by 0.3 rad about z, 0.25 m per column and 0.4 m per row"""
    c, s = np.cos(0.3), np.sin(0.3)
    return qm.frame15([-0.9, -1.7, 0.2], [[c, s, 0], [-s, c, 0], [0, 0, 1]], [0.25, 0.4, 1.0])


def course_params():
    """a gate 0.6 m wide (gate_width is the half width) along the x axis at (0, 0, 1), posts at x = +-0.3; the previous
    waypoint lies 2.6 m out along the gate's line and 2.5 m higher"""
    p = m.QuadrotorMapCostParams()
    p.gate_width = 0.3
    p.track_slop = 0.6
    p.heading_power = 1.5
    p.update_waypoint(2.6, 0.1, 3.5, 0.0)
    p.update_waypoint(0.0, 0.0, 1.0, 0.0)
    return p


# ------------------------------------------------------------------ float64 restatement (shares nothing with the C++) ---
def map64(values, frame, pos):
    """(tex u, tex v, bilinear value with clamp addressing) of the map at a world position"""
    origin, R, res = frame[0:3].astype(np.float64), frame[3:12].astype(np.float64).reshape(3, 3), frame[12:15].astype(np.float64)
    h, w = values.shape
    in_map = R @ (np.asarray(pos, np.float64) - origin)
    u, v = in_map[0] / res[0] / w, in_map[1] / res[1] / h
    qx, qy = np.clip(u * w - 0.5, 0, w - 1), np.clip(v * h - 0.5, 0, h - 1)
    x0, y0 = min(int(np.floor(qx)), w - 2), min(int(np.floor(qy)), h - 2)
    fx, fy = qx - x0, qy - y0
    g = values.astype(np.float64)
    lo = g[y0, x0] * (1 - fx) + g[y0, x0 + 1] * fx
    hi = g[y0 + 1, x0] * (1 - fx) + g[y0 + 1, x0 + 1] * fx
    return u, v, lo * (1 - fy) + hi * fy


def cost64(s, p, crash, values=None, frame=None):
    """(total, crash flag afterwards, sum of the terms' magnitudes, smallest distance of a compared quantity to its threshold)"""
    s = np.asarray(s, np.float64)
    pos, vel, q = s[0:3], s[3:6], s[6:10]
    f = lambda a: np.asarray(a[:], np.float64)  # noqa: E731
    terms, gaps = [], []
    if values is not None:
        u, v, track = map64(values, frame, pos)
        gaps += [abs(u), abs(u - 1), abs(v), abs(v - 1), abs(track - p.track_slop), abs(track - p.track_boundary_cost)]
        outside = u < 0 or u > 1 or v < 0 or v > 1
        terms.append(p.crash_coeff * outside + p.track_coeff * track * (track > p.track_slop) +
                     p.crash_coeff * (track > p.track_boundary_cost))
    left, right = f(p.curr_gate_left)[:2], f(p.curr_gate_right)[:2]
    gate = left - right
    rel = pos[:2] - right
    off_line = rel[0] * gate[1] - rel[1] * gate[0]
    along = rel @ gate / (gate @ gate)
    gaps += [abs(abs(off_line) - p.min_dist_to_gate_side)] + [abs(along - a) for a in (-0.5, 0.0, 1.0, 1.5)]
    hit = abs(off_line) < p.min_dist_to_gate_side and (-0.5 <= along < 0 or 1 < along <= 1.5)
    terms.append(p.crash_coeff * abs(along) * hit)
    cw, pw = f(p.curr_waypoint), f(p.prev_waypoint)
    d1, d2 = np.linalg.norm(pos[:2] - pw[:2]), np.linalg.norm(pos[:2] - cw[:2])
    wanted = (1 - d1 / (d1 + d2 + 0.001)) * pw[2] + (1 - d2 / (d1 + d2 + 0.001)) * cw[2]
    miss = (pos[2] - wanted) ** 2
    gaps.append(abs(miss - p.gate_width))
    terms.append(p.height_coeff * miss + 400 * (miss > p.gate_width))
    dist = np.linalg.norm(pos - cw[:3])
    gaps.append(abs(dist - p.gate_margin))
    flight = (rotation64(q) * (q @ q)) @ vel  # the DCM formulas are not normalised: |q|^2 R
    off = np.arctan2(flight[1], flight[0]) - np.arctan2(cw[1] - pos[1], cw[0] - pos[0])
    off = abs((off + np.pi) % (2 * np.pi) - np.pi)
    # the two directions are ill-conditioned where their vectors are short: kept away from that as from a threshold
    gaps += [np.hypot(flight[0], flight[1]) / 100, np.hypot(cw[0] - pos[0], cw[1] - pos[1]) / 100]
    terms.append(p.heading_coeff * off ** p.heading_power * (dist > p.gate_margin))
    terms.append(p.speed_coeff * (np.hypot(vel[0], vel[1]) - p.desired_speed) ** 2)
    rpy = euler64(q)
    terms.append(p.attitude_coeff * (rpy[0] ** 2 + rpy[1] ** 2))
    crash = 1 if (crash or hit) else 0
    terms.append(p.gate_pass_cost * (dist < p.gate_margin))
    terms.append(crash * p.crash_coeff)
    return float(np.sum(terms)), crash, float(np.sum(np.abs(terms))), float(min(gaps))


# ------------------------------------------------------------------ CPU: known answers on the shipped class -------------
def test_reference_check_speed_cost(host):
    """the reference's checkSpeedCost (tests/cost_functions/quadrotor_map_cost_test.cu): v = (3, 4), speed_coeff 10,
    desired_speed 10 -> 10 (5 - 10)^2 = 250"""
    p = m.QuadrotorMapCostParams()
    p.speed_coeff, p.desired_speed = 10, 10
    host.set_cost_params(p)
    assert host.terms(state([0, 0, 0], [3, 4, 0]))[4] == 250.0
    assert host.terminal_cost(state([1, 2, 3])) == 0.0
    assert host.L.map_cost_max_cost_value() == MAX_COST and host.L.map_cost_traits() == 3


def test_gate_side_branches(host):
    """posts at (0, 0) right and (0, 2) left: the projection is y / 2, the cross product 2 x.  Half a gate beyond the left
    post (1.25) and before the right one (-0.25) are hits of crash_coeff |projection|; 1.5 still is, just beyond it is not;
    between the posts is not; a cross product of 0.6 >= min_dist_to_gate_side = 0.5 is not"""
    p = m.QuadrotorMapCostParams()
    p.update_gate_boundaries(0, 2, 0, 0, 0, 0)
    host.set_cost_params(p)
    gate = lambda x, y: host.terms(state([x, y, 0]))[1]  # noqa: E731
    assert gate(0.1, 2.5) == 1250.0 and gate(0.1, -0.5) == 250.0 and gate(-0.1, -1.0) == 500.0
    assert gate(0.1, 3.0) == 1500.0 and gate(0.1, 3.001) == 0.0 and gate(0.1, -1.001) == 0.0
    assert gate(0.1, 1.0) == 0.0 and gate(0.1, 2.0) == 0.0 and gate(0.1, 0.0) == 0.0
    assert gate(0.3, 2.5) == 0.0 and gate(0.24, 2.5) == 1250.0
    # the crash flag follows the gate term
    assert host.state_cost_crash(state([0.1, 2.5, 0]))[1] == 1 and host.state_cost_crash(state([0.1, 1.0, 0]))[1] == 0


def test_height_branches(host):
    """previous waypoint (0, 0, 1), current (4, 0, 1), vehicle above (1, 0): d1 = 1, d2 = 3, the wanted height
    (1 - 1 / 4.001) + (1 - 3 / 4.001) = 2 - 4 / 4.001.  At z = 3 the squared miss is above gate_width = 2.15: 5 miss + 400;
    at z = 2 it is not: 5 miss"""
    p = m.QuadrotorMapCostParams()
    p.update_waypoint(0, 0, 1, 0)
    p.update_waypoint(4, 0, 1, 0)
    host.set_cost_params(p)
    w1, w2 = float(np.float32(1 / 4.001)), float(np.float32(3 / 4.001))  # the two quotients are rounded to float, the blend is fp64
    wanted = np.float32((1.0 - w1) * 1.0 + (1.0 - w2) * 1.0)
    for z, extra in ((3.0, 400.0), (2.0, 0.0)):
        miss = np.float32(np.float32(z) - wanted) ** 2
        assert (miss > 2.15) == (extra > 0)
        want = np.float32(np.float32(5 * miss) + np.float32(extra))
        assert host.terms(state([1, 0, z]))[2] == want, (z, want)
    assert abs(float(wanted) - (2 - 4 / 4.001)) < 1e-6


def test_gate_pass_heading_and_waypoint_term(host):
    """at the waypoint, level, flying at desired_speed, previous waypoint at height 0: every term is 0 and the cost is
    gate_pass_cost = -150.  0.6 m short of it (gate_margin 0.5) the reward is gone and the heading term is on: flying along +y
    towards a waypoint that lies along +x is a quarter turn, heading_coeff pi / 2.  The waypoint term is computed
    (dist_to_waypoint_coeff d^2) and is not part of the cost"""
    p = m.QuadrotorMapCostParams()
    p.update_waypoint(7, 0, 0, 0)
    p.update_waypoint(2, 1, 3, 0)
    p.dist_to_waypoint_coeff = 2
    host.set_cost_params(p)
    at = state([2, 1, 3], [5, 0, 0])
    assert host.state_cost_crash(at) == (np.float32(-150), 0)
    t = host.terms(at)
    assert t[3] == 0 and t[7] == 0 and t[6] == 0
    near = state([2 - 0.3, 1, 3], [0, 5, 0])  # inside the margin: no heading term whatever the direction of flight
    assert host.terms(near)[3] == 0
    away = state([2 - 0.6, 1, 3], [0, 5, 0])
    t = host.terms(away)
    assert abs(t[3] - 5 * np.pi / 2) < 1e-5 and abs(t[7] - 0.6) < 1e-6 and abs(t[6] - 2 * 0.36) < 1e-5
    total, _ = host.state_cost_crash(away)
    assert abs(total - t[:6].sum()) < 1e-3  # no -150, no waypoint term


def test_heading_power_keeps_powf_values_at_zero(host):
    """flying along +x straight at a waypoint that lies along +x is a heading error of exactly 0.  powf(0, 0) is 1 and powf(0, p)
    is 0 for p > 0; exp(p log 0) alone would give NaN at p == 0 and the step MAX_COST_VALUE.  A quarter turn at power 0 is 1 too"""
    p = m.QuadrotorMapCostParams()
    p.update_waypoint(7, 0, 0, 0)
    p.update_waypoint(2, 1, 3, 0)
    straight, quarter = state([2 - 0.6, 1, 3], [5, 0, 0]), state([2 - 0.6, 1, 3], [0, 5, 0])
    for power, want_straight, want_quarter in ((0.0, 5.0, 5.0), (1.0, 0.0, 5 * np.pi / 2), (2.0, 0.0, 5 * (np.pi / 2) ** 2)):
        p.heading_power = power
        host.set_cost_params(p)
        assert host.terms(straight)[3] == np.float32(want_straight), power
        assert abs(host.terms(quarter)[3] - want_quarter) <= 1e-5 * max(want_quarter, 1), power
        assert np.isfinite(host.state_cost_crash(straight)[0]) and host.state_cost_crash(straight)[0] < MAX_COST, power


def test_costmap_branches(host):
    """a constant map under an identity frame of 1 m cells (7 x 9 m): outside it crash_coeff is added and the clamped map
    still sampled; the value against track_slop = 0.5 (below: nothing, above: track_coeff value) and against
    track_boundary_cost = 2.5 (above: crash_coeff on top)"""
    p = m.QuadrotorMapCostParams()
    p.track_slop = 0.5
    host.set_cost_params(p)
    frame = qm.frame15([0, 0, 0], np.eye(3), [1, 1, 1])
    inside, outside = state([3.5, 4.5, 0]), state([7.5, 4.5, 0])
    try:
        for value, want in ((0.4, 0.0), (0.6, 6.0), (2.4, 24.0), (2.6, 1026.0)):
            host.set_costmap(np.full((9, 7), value, np.float32), frame)
            assert abs(host.terms(inside)[0] - want) <= 1e-5 * max(want, 1), (value, want)
            assert abs(host.terms(outside)[0] - (want + 1000)) <= 1e-5 * (want + 1000), (value, want)
        for pos in ([-0.01, 4.5, 0], [3.5, -0.01, 0], [3.5, 9.01, 0]):
            assert abs(host.terms(state(pos))[0] - 2026) < 0.1
        host.set_costmap(None, None)
        assert host.terms(outside)[0] == 0.0  # without a map the term is 0
    finally:
        host.set_costmap(None, None)


def test_crash_is_sticky_and_nan_is_max_cost(host):
    """a rollout's crash flag, set by a gate-side hit on step t, is charged on that step and on every later one"""
    p = m.QuadrotorMapCostParams()
    p.update_gate_boundaries(0, 2, 0, 0, 0, 0)
    host.set_cost_params(p)
    clear, hit = state([0.1, 1.0, 0]), state([0.1, 2.5, 0])
    crash = 0
    c0, crash = host.state_cost_crash(clear, crash, 0)
    assert crash == 0
    c1, crash = host.state_cost_crash(hit, crash, 1)
    assert crash == 1 and c1 == host.terms(hit)[:6].sum() + np.float32(1000)
    c2, crash = host.state_cost_crash(clear, crash, 2)
    assert crash == 1 and c2 == c0 + np.float32(1000)
    for bad in (0, 2, 4, 7):
        y = clear.copy()
        y[bad] = np.nan
        assert host.state_cost_crash(y)[0] == MAX_COST, bad
    assert np.isfinite(host.state_cost_crash(clear)[0])


# ------------------------------------------------------------------ CPU: shipped class == restatement, bit for bit -------
def course_states(n, seed):
    """states scattered over the course's map and gate: positions within 2 m of the gate, speeds up to 8 m/s"""
    x = random_states(n, seed).astype(np.float64)
    x[:, 0:3] = x[:, 0:3] * [2.2, 1.6, 1.5] + [0.5, 0, 1.5]
    x[:, 3:6] *= 8
    return x.astype(np.float32)


@pytest.mark.parametrize("with_map", [True, False], ids=["map", "no-map"])
def test_shipped_class_equals_restatement_bitwise(host, with_map):
    p = course_params()
    o = qm.QuadrotorMapOracle(4, 3)
    try:
        for power in (1.5, 1.0, 0.0):
            p.heading_power = power
            host.set_cost_params(p)
            o.set_cost_params(p)
            host.set_costmap(track_map() if with_map else None, track_frame())
            o.set_costmap(track_map() if with_map else None, track_frame())
            xs = np.concatenate([course_states(400, 41), [state([0.1, 0.45, 1.0]), state([0, 0, 1], [5, 0, 0]), state([9, 9, 9])]])
            hits = 0
            for i, x in enumerate(xs):
                assert np.array_equal(bits(host.terms(x)), bits(o.terms(x))), (i, host.terms(x), o.terms(x))
                for crash in (0, 1):
                    a, b = host.state_cost_crash(x, crash, i), o.state_cost_crash(x, crash, i)
                    assert bits(a[0]) == bits(b[0]) and a[1] == b[1], (i, crash, a, b)
                hits += host.state_cost_crash(x)[1]
            assert hits > 5
    finally:
        host.set_costmap(None, None)


# ------------------------------------------------------------------ CPU: restatement against float64 --------------------
def test_restatement_against_float64():
    """The CPU restatement against the independent float64 one, on the course's map: relative 1e-4 of the sum of the terms'
    magnitudes (the reward is negative).  The cost jumps at its branch thresholds, so the states are DRAWN at least MARGIN = 1e-3
    from every threshold — both texture coordinates against 0 and 1, the map value against track_slop and track_boundary_cost, the
    cross product against min_dist_to_gate_side, the projection against -0.5 / 0 / 1 / 1.5, the squared height miss against
    gate_width, the distance against gate_margin; the two direction vectors of the heading term at least 0.1 long: the draw
    (float64 side only) replaces a candidate that is closer.  Every state drawn is compared, none is dropped afterwards, and
    the margin is asserted again on the compared set."""
    p = course_params()
    values, frame = track_map(), track_frame()
    o = qm.QuadrotorMapOracle(4, 3)
    o.set_cost_params(p)
    o.set_costmap(values, frame)
    drawn, seed = [], 50
    while len(drawn) < 600:
        for x in course_states(200, seed):
            if cost64(x, p, 0, values, frame)[3] >= MARGIN and len(drawn) < 600:
                drawn.append(x)
        seed += 1
    worst, taken = 0.0, np.zeros(5, int)
    for i, x in enumerate(drawn):
        want, crash64, scale, gap = cost64(x, p, i % 2, values, frame)
        assert gap >= MARGIN
        got, crash = o.state_cost_crash(x, i % 2)
        assert crash == crash64
        worst = max(worst, abs(float(got) - want) / scale)
        u, v, track = map64(values, frame, x[:3])
        t = o.terms(x)
        taken += [not (0 <= u <= 1 and 0 <= v <= 1), track > p.track_boundary_cost, t[1] > 0, t[7] < p.gate_margin, t[2] > 400]
    print("cost against float64: %.3g relative; branches taken %s" % (worst, taken))
    assert (taken > 0).all(), taken
    assert worst <= REL_TOL, worst


# ------------------------------------------------------------------ CPU: parameter block and updateWaypoint -------------
def test_parameter_block_layout_in_c_cpp_and_python(host):
    """size and the offset of every field agree between model_params.h, the plugin's class and the Python mirror; the class's
    defaults, copied out of C++, are the mirror's defaults byte for byte (the NaN end waypoint included)"""
    in_class, in_pod = np.zeros(28, np.int32), np.zeros(28, np.int32)
    assert host.L.map_cost_field_offsets(in_class, in_pod) == 27
    names = [f[0] for f in m.QuadrotorMapCostParams._fields_]
    mirror = [getattr(m.QuadrotorMapCostParams, n).offset for n in names] + [C.sizeof(m.QuadrotorMapCostParams)]
    assert len(names) == 27 and in_class.tolist() == in_pod.tolist() == mirror and mirror[-1] == 4 * 53
    block = m.QuadrotorMapCostParams()
    block.crash_coeff = -1
    host.L.map_cost_default_params(C.byref(block))
    d = m.QuadrotorMapCostParams()
    assert bytes(block) == bytes(d)
    assert list(d.control_cost_coeff) == [1.0] * 4 and d.discount == 1.0 and np.isnan(list(d.end_waypoint)).all()
    assert (d.attitude_coeff, d.crash_coeff, d.dist_to_waypoint_coeff, d.heading_coeff, d.heading_power) == (10, 1000, 0, 5, 1)
    assert (d.height_coeff, d.track_coeff, d.speed_coeff, d.track_slop, d.gate_pass_cost) == (5, 10, 5, 0, -150)
    assert (d.desired_speed, d.gate_margin, d.min_dist_to_gate_side, d.track_boundary_cost) == (5, 0.5, 0.5, 2.5)
    assert d.gate_width == np.float32(2.15)


def test_update_waypoint_shuffle_and_no_change_rule(host):
    """QuadrotorMapCostParams::updateWaypoint: the new waypoint pushes the current one (and its posts) to previous and places
    the posts gate_width to either side along the heading; the same waypoint again is no update and shuffles nothing.  The Python
    mirror gives the C++ class's bytes (cosf / sinf in float32)"""
    py, cc = m.QuadrotorMapCostParams(), m.QuadrotorMapCostParams()
    for wp in ((1.5, -2.0, 3.0, 0.7), (4.0, 1.0, 2.5, -2.1), (4.0, 1.0, 2.5, -2.1), (4.0, 1.0, 2.5, 0.0), (-3.0, 0.2, 1.0, 3.0)):
        before = bytes(py)
        changed = py.update_waypoint(*wp)
        assert changed == bool(host.L.map_cost_update_waypoint(C.byref(cc), *wp))
        assert bytes(py) == bytes(cc), wp
        if not changed:
            assert bytes(py) == before
    assert list(py.prev_waypoint) == [4.0, 1.0, 2.5, 0.0] and list(py.curr_waypoint) == [-3.0, np.float32(0.2), 1.0, 3.0]
    p = m.QuadrotorMapCostParams()
    assert p.update_waypoint(1, 2, 3, np.pi / 2) and not p.update_waypoint(1, 2, 3, np.pi / 2)
    assert np.allclose(list(p.curr_gate_left), [1, 2 + 2.15, 3], atol=1e-6) and np.allclose(list(p.curr_gate_right), [1, 2 - 2.15, 3], atol=1e-6)
    assert list(p.prev_waypoint) == [0] * 4 and list(p.prev_gate_left) == [0] * 3
    old_left, old_right = list(p.curr_gate_left), list(p.curr_gate_right)
    assert p.update_waypoint(5, 5, 5, 0)
    assert list(p.prev_waypoint)[:3] == [1, 2, 3] and list(p.prev_gate_left) == old_left and list(p.prev_gate_right) == old_right
    # the posts alone
    lr = np.array([1, 2, 3, 4, 5, 6], np.float32)
    assert p.update_gate_boundaries(*lr) == bool(host.L.map_cost_update_gate(C.byref(cc), lr)) and not p.update_gate_boundaries(*lr)
    assert list(p.curr_gate_right) == [4, 5, 6] and list(p.prev_gate_left) == [5 + np.float32(2.15), 5, 5]


# ------------------------------------------------------------------ CPU: registration ----------------------------------
def test_registration(quadrotor_map):
    import quadrotor_oracle as qo
    assert m.list_models().count("quadrotor_map") == 1
    qm.load_model(m)  # a second load is a no-op
    assert m.list_models().count("quadrotor_map") == 1
    d = m.describe_model("quadrotor_map")
    assert d["shapes"] == [(64, 1, 1), (64, 1, 2), (32, 4, 1), (16, 1, 1)] and d["pipeline"] and not d["rmppi"]
    assert d["replicated_lane_shapes"] == [] and d["streamed_merge"]
    assert m.describe_model("quadrotor_map", m.MPPI_SAMPLER_COLORED) is None
    # "quadrotor" beside it is what it was
    qo.load_model(m)
    q = m.describe_model("quadrotor")
    assert q["shapes"] == [(64, 1, 1), (64, 1, 2), (32, 4, 1), (16, 1, 1)] and q["pipeline"] and not q["rmppi"]
    assert q["replicated_lane_shapes"] == [] and q["streamed_merge"] and m.list_models().count("quadrotor") == 1
    assert {k: v for k, v in d.items() if k != "name"} == {k: v for k, v in q.items() if k != "name"}


# ------------------------------------------------------------------ configurations of the GPU tests ---------------------
def map_cfg(K=192, T=7, D=1, with_map=True, num_iters=1, lambda_=40.0):
    """The vehicle starts 0.9 m out along the gate's line — beyond the left post, off the map and 0.8 m below the height wanted
    there — tilted, on the q_w < 0 sheet, and flies down that line at 8 m/s: it comes onto the map over its high edge, passes
    beyond the left post (a gate-side hit on step 1, not on step 0), then through the gate's margin, and at T = 33 out past the
    right post and off the map's other edge.  Thrust noise of 12 N leaves [0, 36] on both sides."""
    q0 = -quat_from_rpy64(0.2, -0.15, 3.0)
    x0 = np.concatenate([[0.9, 0.1, 1.05], [-8.0, 0.3, -0.4], q0, [0.2, -0.4, 0.1]]).astype(np.float32)
    cfg = dict(model="quadrotor_map", K=K, T=T, D=D, dt=0.02, lambda_=lambda_, alpha=0.1, num_iters=num_iters,
               dyn=m.QuadrotorDynamicsParams(1.3), cost=course_params(), ranges=None, std_dev=[2.0, 2.0, 2.0, 12.0],
               control_cost_coeff=[2.0, 2.0, 2.0, 0.3], x0=x0, oracle=make_map_oracle)
    if with_map:
        cfg["blobs"] = {"costmap_transform": track_frame(), "costmap": track_map()}
    return cfg


def make_map_oracle(cfg):
    o = qm.QuadrotorMapOracle(cfg["K"], cfg["T"], cfg["D"], cfg["dt"], cfg["lambda_"], cfg["alpha"], cfg["num_iters"])
    o.set_dynamics_params(cfg["dyn"])
    o.set_cost_params(cfg["cost"])
    blobs = cfg.get("blobs", {})
    o.set_costmap(blobs.get("costmap"), blobs.get("costmap_transform"))
    o.set_sampler(cfg["std_dev"], cfg["control_cost_coeff"], cfg.get("pure_pct", 0.01), cfg.get("decay", 1.0))
    return o


def nominal_control(T):
    u = np.zeros((T, 4), np.float32)
    u[:, 3] = 9.81
    u[1::3, 3] = 2.0
    u[2::3, 3] = 33.0
    u[:, 0] = 0.1
    return u


_REFERENCE = {}


def _reference_run(K, T, with_map=True):
    """two consecutive calls of the CPU restatement with a slide between, computed once per (K, T, map) and shared; with the
    map, the branch census of the first call is asserted here"""
    key = (K, T, with_map)
    if key not in _REFERENCE:
        cfg = map_cfg(K=K, T=T, with_map=with_map)
        o = make_map_oracle(cfg)
        o.set_nominal_control(nominal_control(T))
        eps = [host_noise(1, K, T, 4, seed=K + T + i) for i in range(2)]
        x1 = o.model_step(cfg["x0"], nominal_control(T)[0])[0]
        calls = []
        for i, x in enumerate((cfg["x0"], x1)):
            mean = o.control().copy()
            o.vanilla_compute_control(x, 1, eps[i])
            calls.append(dict(x=x, eps=eps[i], mean=mean, costs=o.costs().copy(), control=o.control().copy(), samples=o.samples().copy()))
            o.vanilla_slide(1)
        for c in calls:
            c["costs"].setflags(write=False)
        assert calls[0]["samples"][..., 3].min() == 0.0 and calls[0]["samples"][..., 3].max() == 36.0 and cfg["x0"][6] < 0
        _REFERENCE[key] = calls
    return _REFERENCE[key]


def test_gpu_inputs_take_every_branch():
    """what the GPU comparison is worth: counted on the restatement, over the rollout-steps of the first call at (192, 7) and at
    (100, 33) each, at least one step left the map, one sampled a map value above track_boundary_cost, one hit a gate side, one
    passed the gate, one had the heading term on and one off, one took the +400 height branch; and a rollout's crash flag was
    set strictly after step 0 and before the last step"""
    for K, T in ((192, 7), (100, 33)):
        cfg = map_cfg(K=K, T=T)
        o = make_map_oracle(cfg)
        counts, first = o.census(cfg["x0"], _reference_run(K, T)[0]["samples"][0])
        print("K=%d T=%d: %s; first crash steps %s" % (K, T, counts, np.unique(first)))
        assert all(v > 0 for v in counts.values()), (K, T, counts)
        assert ((first > 0) & (first < T - 1)).any(), (K, T, np.unique(first))
        assert sum(counts.values()) - counts["heading_on"] - counts["heading_off"] < 5 * K * T  # counted per rollout-step


# ------------------------------------------------------------------ GPU: every form ------------------------------------
FORMS = [("fused64x1x1", (64, 1, 1), m.MPPI_KERNEL_FUSED), ("pipeline64x1x1", (64, 1, 1), m.MPPI_KERNEL_PIPELINE),
         ("fused32x4x1", (32, 4, 1), m.MPPI_KERNEL_FUSED), ("fused16x1x1", (16, 1, 1), m.MPPI_KERNEL_FUSED)]


def test_forms_follow_kernel_forms(quadrotor_map):
    from kernel_forms import pipeline_family
    d = m.describe_model("quadrotor_map")
    want = []
    for sh in d["shapes"]:
        if sh[2] == 1:
            want.append(("fused%dx%dx%d" % sh, sh, m.MPPI_KERNEL_FUSED))
            if pipeline_family(d, sh):
                want.append(("pipeline%dx%dx%d" % sh, sh, m.MPPI_KERNEL_PIPELINE))
    assert want == FORMS
    assert pipeline_family(d, (64, 1, 2)) == "pipeline"


_COSTS_64x1x1 = {}


def _hold_two_calls(eng, calls, T, tag0, expect):
    """the two calls of _reference_run with a slide between on one handle: trajectory costs 0 ulp, clamped samples 0 ulp, u* within
    1e-5, and every form gives (64,1,1)'s costs bit for bit; expect(info, tag) checks which kernel form ran"""
    eng.updateImportanceSampler(nominal_control(T))
    for i, c in enumerate(calls):
        tag = "%s call %d" % (tag0, i)
        if i > 0:
            # the slid u* is the next mean; hold it to the u* bar, then start both sides from the same mean
            assert np.abs(eng.getControlSeq() - c["mean"]).max() <= U_TOL, tag
            eng.updateImportanceSampler(c["mean"])
        eng.injectNoise(c["eps"])
        eng.computeControl(c["x"], 1)
        expect(eng.getLaunchInfo(), tag)
        costs = eng.getSampledCostSeq()
        dc = int(ulp_diff(costs, c["costs"]).max())
        du = float(np.abs(eng.getControlSeq() - c["control"]).max())
        dv = int(ulp_diff(eng.getSampledControls(), c["samples"]).max())
        print("%s: costs %d ulp, samples %d ulp, u* %.3g" % (tag, dc, dv, du))
        assert dc == 0, "%s: costs differ by up to %d ulp" % (tag, dc)
        assert dv == 0, "%s: clamped samples differ by up to %d ulp" % (tag, dv)
        assert du <= U_TOL, "%s: u* differs by %g" % (tag, du)
        first = _COSTS_64x1x1.setdefault((len(c["costs"][0]), T, i), costs.copy())
        assert np.array_equal(bits(costs), bits(first)), tag
        eng.slideControlSequence(1)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_every_form_against_restatement(gpu, quadrotor_map, form):
    """K = 192 (three blocks of 64) and K = 100 (a partial block), T = 7 and 33, injected noise, two calls with a slide between:
    trajectory costs 0 ulp, clamped samples 0 ulp, u* within 1e-5; every form gives (64,1,1)'s costs bit for bit"""
    name, shape, variant = form

    def expect(info, tag):
        assert info["block"] == shape and info["family"] == ("fused" if variant == m.MPPI_KERNEL_FUSED else "pipeline"), (tag, info)
        assert not info["rows_in_hbm"] and not info["streamed_merge"], (tag, info)
    for K, T in ((192, 7), (100, 33)):
        eng = make_engine(map_cfg(K=K, T=T), block_x=shape[0], block_y=shape[1], kernel_variant=variant, save_samples=True)
        try:
            _hold_two_calls(eng, _reference_run(K, T), T, "%s K=%d T=%d" % (name, K, T), expect)
        finally:
            eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [m.MPPI_KERNEL_FUSED, m.MPPI_KERNEL_PIPELINE], ids=["fused", "pipeline"])
def test_rows_in_hbm_forms(gpu, quadrotor_map, variant):
    """MPPI_AMD_ROWS_IN_HBM=1: the sample rows in HBM instead of LDS, the forms a long horizon runs, at K = 100, T = 33; the same
    two calls, to the same bars"""
    from kernel_forms import env_override
    K, T = 100, 33

    def expect(info, tag):
        assert info["rows_in_hbm"] and info["block"] == (64, 1, 1), (tag, info)
        assert info["family"] == ("fused" if variant == m.MPPI_KERNEL_FUSED else "pipeline"), (tag, info)
    with env_override(MPPI_AMD_ROWS_IN_HBM="1"):
        eng = make_engine(map_cfg(K=K, T=T), block_x=64, block_y=1, kernel_variant=variant, save_samples=True)
    try:
        _hold_two_calls(eng, _reference_run(K, T), T, "rows in HBM, %s" % ("fused" if variant == m.MPPI_KERNEL_FUSED else "pipeline"), expect)
    finally:
        eng.close()


_TUBE = {}


def _tube_reference(K=128, T=20):
    """two Tube calls of the restatement with a slide between, computed once.  Before the second call both of its means are set to
    the slid real-system u* (so that the engine can start from the very same mean), and its nominal state is its own"""
    if not _TUBE:
        cfg = map_cfg(K=K, T=T, D=2)
        o = make_map_oracle(cfg)
        o.set_nominal_control(nominal_control(T))
        x1 = o.model_step(cfg["x0"], nominal_control(T)[0])[0]
        calls = []
        for i, x in enumerate((cfg["x0"], x1)):
            eps = host_noise(1, K, T, 4, seed=5 + i)
            mean = o.control().copy()
            if i > 0:
                o.set_nominal_control(mean)
            o.tube_compute_control(x, 1, eps)
            calls.append(dict(x=x, eps=eps, mean=mean, costs=o.costs().copy(), samples=o.samples().copy(), control=o.control().copy(),
                              nominal_control=o.nominal_control().copy(), nominal_used=o.stats()["nominal_state_used"]))
            o.tube_slide(1)
        _TUBE["cfg"], _TUBE["calls"] = cfg, calls
    return _TUBE["cfg"], _TUBE["calls"]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [m.MPPI_KERNEL_FUSED, m.MPPI_KERNEL_PIPELINE, m.MPPI_KERNEL_AUTO], ids=["fused", "pipeline", "auto-fold"])
def test_tube(gpu, quadrotor_map, variant):
    """Shape<64,1,2> at K = 128, T = 20 in both families, and the folded form (32,1,2) a Tube controller without a block shape
    picks; two calls with a slide between against the restatement's Tube computeControl: trajectory costs and clamped samples
    of both systems 0 ulp, u* and nominal u* within 1e-5, on both calls"""
    cfg, calls = _tube_reference()
    kw = {} if variant == m.MPPI_KERNEL_AUTO else dict(block_x=64, block_y=1)
    eng = make_engine(cfg, kernel_variant=variant, save_samples=True, **kw)
    try:
        eng.updateImportanceSampler(nominal_control(20))
        for i, c in enumerate(calls):
            if i > 0:
                assert np.abs(eng.getControlSeq() - c["mean"]).max() <= U_TOL, i
                eng.updateImportanceSampler(c["mean"])
            eng.injectNoise(c["eps"])
            eng.computeControl(c["x"], 1)
            info = eng.getLaunchInfo()
            if variant == m.MPPI_KERNEL_AUTO:
                assert info["family"] == "pipeline_fold" and info["block"] == (32, 1, 2), info
            else:
                assert info["block"] == (64, 1, 2), info
                assert info["family"] == ("fused" if variant == m.MPPI_KERNEL_FUSED else "pipeline"), info
            costs = eng.getSampledCostSeq()
            d = [int(ulp_diff(costs[z], c["costs"][z]).max()) for z in range(2)]
            dv = int(ulp_diff(eng.getSampledControls(), c["samples"]).max())
            du = float(np.abs(eng.getControlSeq() - c["control"]).max())
            dn = float(np.abs(eng.getNominalControlSeq() - c["nominal_control"]).max())
            print("tube call %d: costs %s ulp, samples %d ulp, u* %.3g, nominal u* %.3g, nominal state used %s" % (i, d, dv, du, dn, c["nominal_used"]))
            assert dv == 0, i
            assert d == [0, 0], (i, d)
            if i == 0:
                assert np.array_equal(bits(costs[0]), bits(costs[1]))
            assert du <= U_TOL and dn <= U_TOL, (i, du, dn)
            eng.slideControlSequence(1)
    finally:
        eng.close()


def _philox_call(cfg, T, mean, eps, expect, tag, **engine_kw):
    """one one-iteration computeControl with the in-kernel Philox draw (eps is the same stream, evaluated on the host) from `mean`:
    trajectory costs and clamped samples 0 ulp against the restatement; returns (engine's u*, engine's costs, restatement's u*)"""
    eng = make_engine(cfg, save_samples=True, **engine_kw)
    try:
        eng.updateImportanceSampler(nominal_control(T))
        eng.setSeed(PHILOX_SEED)
        eng.computeControl(cfg["x0"], 1)
        expect(eng.getLaunchInfo())
        o = make_map_oracle(dict(cfg, num_iters=1))
        o.set_nominal_control(mean)
        o.vanilla_compute_control(cfg["x0"], 1, eps[None])
        costs = eng.getSampledCostSeq()
        dc, dv = int(ulp_diff(costs, o.costs()).max()), int(ulp_diff(eng.getSampledControls(), o.samples()).max())
        print("%s: costs %d ulp, samples %d ulp" % (tag, dc, dv))
        assert dc == 0, "%s: costs differ by up to %d ulp" % (tag, dc)
        assert dv == 0, "%s: clamped samples differ by up to %d ulp" % (tag, dv)
        return eng.getControlSeq(), costs, o.control()
    finally:
        eng.close()


@pytest.mark.gpu
def test_philox_in_the_loop_forms(gpu, quadrotor_map):
    """the kernels that draw their noise themselves are compilations of the cost wave of their own: one iteration at K = 200,
    T = 8 on the one-lane pipeline, on its rows-in-HBM form and fused, trajectory costs and clamped samples 0 ulp against the
    restatement on the same Philox stream, u* within 1e-5, and the three forms' costs the same bits"""
    from kernel_forms import env_override
    K, T = 200, 8
    cfg = map_cfg(K=K, T=T)
    eps = po.philox_normal(PHILOX_SEED, 0, K, T, 4)
    seen = []
    for family, hbm, variant in (("pipeline", False, m.MPPI_KERNEL_PIPELINE), ("pipeline", True, m.MPPI_KERNEL_PIPELINE),
                                 ("fused", False, m.MPPI_KERNEL_FUSED)):
        def expect(info):
            assert info["family"] == family and info["rows_in_hbm"] == hbm and info["block"] == (64, 1, 1), info
            assert not info["streamed_merge"], info
        with env_override(MPPI_AMD_ROWS_IN_HBM="1" if hbm else "0"):
            u, costs, want_u = _philox_call(cfg, T, nominal_control(T), eps, expect, "philox %s%s" % (family, ", rows in HBM" if hbm else ""),
                                            block_x=64, block_y=1, kernel_variant=variant)
        assert np.abs(u - want_u).max() <= U_TOL, (family, hbm)
        seen.append(costs)
    assert all(np.array_equal(bits(seen[0]), bits(c)) for c in seen[1:])


@pytest.mark.gpu
def test_streamed_merge_form(gpu, quadrotor_map):
    """two iterations with in-kernel Philox noise on the (64,1,1) pipeline: the second launch merges the first one's block
    records in its sampler waves and is the STREAM_MERGE compilation of the cost wave.  u* against the restatement's two
    iterations on the same stream within 1e-5.

    The costs and clamped samples a handle returns are the LAST iteration's, and that iteration starts from the mean the engine
    merged after the first: within 1e-5 of the restatement's and not its bits, and no call returns it (u* is smoothed and
    clamped after the loop).  Costs in the thousands move by many ulp under a 1e-5 change of the mean, so the restatement cannot
    hold them at 0 ulp directly.  They are held in two links instead: the streamed handle's costs, samples and u* are, bit for
    bit, those of a handle that merges with the merge kernel between its two launches (MPPI_AMD_NO_STREAM_MERGE=1; one merge
    function, so the same mean), whose launches are the plain Philox-in-the-loop kernel, and that kernel's costs and samples are
    0 ulp from the restatement in test_philox_in_the_loop_forms"""
    from kernel_forms import env_override
    K, T = 200, 8
    cfg = map_cfg(K=K, T=T, num_iters=2)
    form = dict(block_x=64, block_y=1, kernel_variant=m.MPPI_KERNEL_PIPELINE, save_samples=True)
    streamed = make_engine(cfg, **form)
    with env_override(MPPI_AMD_NO_STREAM_MERGE="1"):
        plain = make_engine(cfg, **form)
    try:
        for eng in (streamed, plain):
            eng.updateImportanceSampler(nominal_control(T))
            eng.setSeed(PHILOX_SEED)
            eng.computeControl(cfg["x0"], 1)
            info = eng.getLaunchInfo()
            assert info["family"] == "pipeline" and not info["rows_in_hbm"] and info["streamed_merge"] == (eng is streamed), info
        assert streamed.launchCounts() == (2, 1) and plain.launchCounts() == (2, 2)
        dc = int(ulp_diff(streamed.getSampledCostSeq(), plain.getSampledCostSeq()).max())
        dv = int(ulp_diff(streamed.getSampledControls(), plain.getSampledControls()).max())
        print("streamed merge against the two-launch form: costs %d ulp, samples %d ulp" % (dc, dv))
        assert np.array_equal(bits(streamed.getSampledCostSeq()), bits(plain.getSampledCostSeq())), dc
        assert np.array_equal(bits(streamed.getSampledControls()), bits(plain.getSampledControls())), dv
        assert np.array_equal(bits(streamed.getControlSeq()), bits(plain.getControlSeq()))
        o = make_map_oracle(cfg)
        o.set_nominal_control(nominal_control(T))
        eps = np.stack([po.philox_normal(PHILOX_SEED, g, K, T, 4) for g in range(2)])
        o.vanilla_compute_control(cfg["x0"], 1, eps)
        du = float(np.abs(streamed.getControlSeq() - o.control()).max())
        print("streamed merge: u* %.3g" % du)
        assert du <= U_TOL, du
    finally:
        streamed.close()
        plain.close()


# ------------------------------------------------------------------ GPU: the map, the blobs, the parameters -------------
@pytest.mark.gpu
def test_runs_without_a_map_and_the_map_changes_the_costs(gpu, quadrotor_map):
    """without the blobs the run succeeds and equals the restatement without a map; the map, set on the same handle afterwards,
    changes the costs to the restatement's with it"""
    K, T = 100, 33
    bare, mapped = _reference_run(K, T, with_map=False)[0], _reference_run(K, T)[0]
    assert not np.array_equal(bare["costs"], mapped["costs"])
    eng = make_engine(map_cfg(K=K, T=T, with_map=False), save_samples=True)
    try:
        eng.updateImportanceSampler(nominal_control(T))
        eng.injectNoise(bare["eps"])
        eng.computeControl(bare["x"], 1)
        assert int(ulp_diff(eng.getSampledCostSeq(), bare["costs"]).max()) == 0
        assert np.abs(eng.getControlSeq() - bare["control"]).max() <= U_TOL
        m.set_cost_texture(eng, track_map(), track_frame()[0:3], track_frame()[3:12], track_frame()[12:15])
        eng.updateImportanceSampler(nominal_control(T))
        eng.injectNoise(mapped["eps"])
        eng.computeControl(mapped["x"], 1)
        assert int(ulp_diff(eng.getSampledCostSeq(), mapped["costs"]).max()) == 0
        assert np.abs(eng.getControlSeq() - mapped["control"]).max() <= U_TOL
    finally:
        eng.close()


def _refused(eng, name, array, count=None, dims=None):
    a = np.ascontiguousarray(array, np.float32)
    dims = a.shape if dims is None else dims
    st = eng._lib.mppi_set_model_blob(eng._h, name.encode(), a.reshape(-1), a.size if count is None else count,
                                      (C.c_int * len(dims))(*dims), len(dims))
    return st, (eng._lib.mppi_last_error(eng._h) or b"").decode()


@pytest.mark.gpu
def test_blob_refusals(gpu, quadrotor_map):
    """wrong dims or count for either blob: MPPI_ERR_INVALID_ARG with the message of the elevation-map blobs' style; models
    without a cost texture answer as they always did"""
    import quadrotor_oracle as qo
    from common import cartpole_cfg
    qo.load_model(m)
    eng = make_engine(map_cfg(K=64, T=4, with_map=False))
    try:
        want = "costmap: dims must be {height, width} with height*width == count"
        for kw in (dict(array=np.zeros(63)), dict(array=np.zeros((9, 7, 1))), dict(array=np.zeros((9, 7)), count=62),
                   dict(array=np.zeros((9, 7)), dims=(9, 0)), dict(array=np.zeros((9, 7)), dims=(7, 8))):
            st, msg = _refused(eng, "costmap", **kw)
            assert st == m.MPPI_ERR_INVALID_ARG and msg.endswith(want), (kw, st, msg)
        for n in (14, 16, 9):
            st, msg = _refused(eng, "costmap_transform", np.zeros(n))
            assert st == m.MPPI_ERR_INVALID_ARG, n
            assert msg.endswith("costmap_transform: expected 15 floats (origin[3], rotations[9], resolution[3])"), msg
        st, msg = _refused(eng, "elevation_map", np.zeros((9, 7)))
        assert st == m.MPPI_ERR_INVALID_ARG and msg.endswith("model has no blob named 'elevation_map'"), msg
        # a refused blob leaves the handle without a map, and it still runs
        eng.computeControl(map_cfg()["x0"], 1)
    finally:
        eng.close()
    from test_quadrotor import quadrotor_cfg
    for cfg, name, arr in ((quadrotor_cfg(K=64, T=4), "costmap_transform", np.zeros(15)), (quadrotor_cfg(K=64, T=4), "costmap", np.zeros((9, 7))),
                           (cartpole_cfg(K=64, T=4), "costmap", np.zeros((9, 7))), (cartpole_cfg(K=64, T=4), "costmap_transform", np.zeros(15))):
        eng = make_engine(cfg)
        try:
            st, msg = _refused(eng, name, arr)
            assert st == m.MPPI_ERR_INVALID_ARG and msg.endswith("model has no blob named '%s'" % name), (cfg["model"], msg)
        finally:
            eng.close()


@pytest.mark.gpu
def test_waypoint_moves_between_two_calls_on_one_handle(gpu, quadrotor_map):
    """update_waypoint + setCostParams between two computeControl calls, no re-creation: the second call's costs are the
    restatement's with the new waypoint and with previous = the old current one (the map stays set across setCostParams)"""
    K, T = 100, 33
    cfg = map_cfg(K=K, T=T)
    o = make_map_oracle(cfg)
    eng = make_engine(cfg, save_samples=True)
    try:
        p = cfg["cost"]
        old = list(p.curr_waypoint)
        costs = []
        for call in range(2):
            if call == 1:
                assert p.update_waypoint(0.4, -1.6, 1.4, 0.5) and list(p.prev_waypoint) == old
                eng.setCostParams(p)
                o.set_cost_params(p)
            eps = host_noise(1, K, T, 4, seed=70 + call)
            for side in (eng, o):
                (side.updateImportanceSampler if side is eng else side.set_nominal_control)(nominal_control(T))
            eng.injectNoise(eps)
            eng.computeControl(cfg["x0"], 1)
            o.vanilla_compute_control(cfg["x0"], 1, eps)
            costs.append(o.costs().copy())
            assert int(ulp_diff(eng.getSampledCostSeq(), o.costs()).max()) == 0, call
            assert np.abs(eng.getControlSeq() - o.control()).max() <= U_TOL, call
        # the second call is not the first one's costs with other noise only: same noise, old waypoint, other costs
        o2 = make_map_oracle(map_cfg(K=K, T=T))
        o2.set_nominal_control(nominal_control(T))
        o2.vanilla_compute_control(cfg["x0"], 1, host_noise(1, K, T, 4, seed=71))
        assert not np.array_equal(o2.costs(), costs[1])
    finally:
        eng.close()


@pytest.mark.gpu
def test_colored_and_robust_are_refused(gpu, quadrotor_map):
    """as for "quadrotor": both controllers are refused with a message, and no handle comes back"""
    with pytest.raises(m.MPPIError) as e:
        m.ColoredMPPIController("quadrotor_map", 64, 8, 0.01, 1.0)
    assert e.value.status == m.MPPI_ERR_UNSUPPORTED
    assert str(e.value).endswith("mppi_create: model 'quadrotor_map' has no colored-noise instantiation"), str(e.value)
    with pytest.raises(m.MPPIError) as e:
        m.RobustMPPIController("quadrotor_map", 288, 8, 0.01, 1.0)
    assert e.value.status == m.MPPI_ERR_UNSUPPORTED
    assert str(e.value).endswith("mppi_create: model 'quadrotor_map' is not instantiated for Robust MPPI"), str(e.value)
