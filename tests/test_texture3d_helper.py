"""ThreeDTextureHelper (include/mppi_amd/utils/texture_helpers/three_d_texture_helper.hpp) and mppi_texture3d_query.

CPU: the restatement (tests/texture3d_oracle) against the reference's own known answers (TestCPUQuery, CheckCPUWrapping of
tests/texture_helpers/three_d_texture_helper_test.cu) and against a float64 trilinear restatement written here; the shipped helper's
host form against the restatement bit for bit; the z wrap's closed form against the reference's loops; the host class as the
reference's UpdateTexture, UpdateTextureColumnMajor, UpdateTextureException and CopyDataToGPUSplitMiddle tests use it; the stand-alone
host program under the address and undefined-behaviour sanitizers.
GPU: mppi_texture3d_query against the restatement bit for bit, and a layer update through the host class on the device."""
import itertools
import re
import subprocess

import numpy as np
import pytest

import mppi_generic_amd as m
import native_build as nb
import texture3d_oracle as t3
from restate64 import bits

FLOAT_EQ_ULPS = 4  # gtest's EXPECT_FLOAT_EQ


def reference_volume(width, height, depth):
    """the reference tests' data: texel i of layer z holds (z * width * height + i) + channel"""
    base = np.arange(depth * height * width, dtype=np.float32).reshape(depth, height, width)
    return np.stack([base, base + 1, base + 2, base + 3], axis=-1)


def assert_float_eq(got, want):
    want = np.float32(want)
    assert abs(np.float32(got) - want) <= FLOAT_EQ_ULPS * np.spacing(max(abs(want), np.float32(1e-30))), (got, want)


# ------------------------------------------------------------------ CPU: the reference's known answers -------------------
def test_restatement_on_the_reference_cpu_query_answers():
    """TestCPUQuery: 10 x 20 x 5 float4, clamp, linear; its 23 points and expectations, literally"""
    data = reference_volume(10, 20, 5)
    pts = ([(x, 0, 0) for x in (0.0, 0.05, 0.95, 1.0, 0.45, 0.5, 0.55)] +
           [(0, y, 0) for y in (0.025, 0.05, 0.075, 0.975, 1.0, 0.475, 0.5, 0.525)] +
           [(0, 0, z) for z in (0.1, 0.2, 0.3, 1.0, 0.9, 0.8, 0.7, 1.2)])
    want_x = [0, 0, 9, 9, 4, 4.5, 5, 0, 5, 10, 190, 190, 90, 95, 100, 0, 100, 200, 800, 800, 700, 600, 800]
    assert len(pts) == len(want_x) == 23
    for q in (t3.query, t3.helper_query):
        got = q(data, pts)
        for i, w in enumerate(want_x):
            assert_float_eq(got[i, 0], w)
        for i in range(7):  # the test checks all four channels of its first seven points
            for ch in range(4):
                assert_float_eq(got[i, ch], want_x[i] + ch)


def test_restatement_on_the_reference_cpu_wrapping_answers():
    """CheckCPUWrapping: 10 x 20 x 2 float4, wrap on z (period depth - 1 = 1)"""
    data = reference_volume(10, 20, 2)
    pts = [(0, 0, z) for z in (0.0, 0.25, 0.5, 0.75, 1.0)]
    for q in (t3.query, t3.helper_query):
        got = q(data, pts, address_mode=(t3.CLAMP, t3.CLAMP, t3.WRAP))
        for g, w in zip(got[:, 0], (100.0, 0, 100, 200, 100)):
            assert_float_eq(g, w)


# ------------------------------------------------------------------ CPU: float64 ---------------------------------------
def trilinear64(data, pts):
    """float64 trilinear interpolation of data [d][h][w] at texture coordinates pts, clamp addressing.  The texel coordinate
    q = p * extent - 0.5 is taken in float32, the same two IEEE operations as the formula under test, so that what is compared
    is the interpolation; everything after it is float64."""
    d, h, w = data.shape
    out = np.zeros(len(pts))
    D = data.astype(np.float64)
    for n, p in enumerate(np.asarray(pts, np.float32)):
        q = [np.float64(np.clip(np.float32(np.float32(p[a] * np.float32(e)) - np.float32(0.5)), 0, e - 1)) for a, e in enumerate((w, h, d))]
        lo = [int(min(np.floor(q[a]), e - 2)) for a, e in enumerate((w, h, d))]
        f = [q[a] - lo[a] for a in range(3)]
        acc = 0.0
        for cz, cy, cx in itertools.product((0, 1), repeat=3):
            wgt = (f[0] if cx else 1 - f[0]) * (f[1] if cy else 1 - f[1]) * (f[2] if cz else 1 - f[2])
            acc += wgt * D[lo[2] + cz, lo[1] + cy, lo[0] + cx]
        out[n] = acc
    return out


def test_restatement_against_float64():
    """Bound.  One blend is fl(fl(a * fl(1 - d)) + fl(b * d)) with 0 <= d <= 1 and |a|, |b| <= M = max(|lo|, |hi|): with
    u = 2^-24, fl(1 - d) carries one relative error, each product one more, the sum one more, so the blend is off its exact value by
    at most ((1 - d) 3 u + d 2 u) M <= 3 u M, and it stays within [lo, hi] to that order.  The three nested levels (x, y, z) are convex
    combinations, which pass an input error on unamplified and add their own: 3 u M, 6 u M, 9 u M.  Rounding the float64 answer
    to float32 for the comparison is not needed (the difference is taken in float64).  Bar: 9 * 2^-24 * M, which is below 9 ulp(M)
    (ulp(M) > 2^-24 M).  The observed maximum is printed (DESIGN.md has it)."""
    rng = np.random.default_rng(31)
    worst = 0.0
    for lo_v, hi_v in ((-3.0, 5.0), (100.0, 104.0), (-1e-3, 1e-3)):
        data = rng.uniform(lo_v, hi_v, (5, 3, 4)).astype(np.float32)
        pts = rng.uniform(-0.1, 1.1, (4000, 3)).astype(np.float32)
        M = max(abs(lo_v), abs(hi_v))
        got = t3.query(data, pts)[:, 0].astype(np.float64)
        err = np.abs(got - trilinear64(data, pts)).max() / (2.0 ** -24 * M)
        worst = max(worst, err)
        assert err <= 9.0, (lo_v, hi_v, err)
    print("trilinear restatement: worst error %.3f x 2^-24 max(|lo|, |hi|) (bar 9)" % worst)


# ------------------------------------------------------------------ cases shared by the CPU and the GPU comparison ---------
W, H, D = 4, 3, 5  # three different extents, so that a swapped axis shows
FRAME = t3.frame15([1.0, -2.0, 0.5], [0, 1, 0, -1, 0, 0, 0, 0, 1], [0.5, 0.25, 2.0])
BORDER_COLOR = (-7.0, -8.0, -9.0, -10.0)
ADDRESSING = [(t3.CLAMP,) * 3, (t3.BORDER, t3.CLAMP, t3.CLAMP), (t3.CLAMP, t3.BORDER, t3.CLAMP), (t3.CLAMP, t3.CLAMP, t3.BORDER),
              (t3.BORDER,) * 3, (t3.CLAMP, t3.CLAMP, t3.WRAP), (t3.BORDER, t3.CLAMP, t3.WRAP)]


def volume(depth=D, channels=1):
    rng = np.random.default_rng(7 + depth + channels)
    v = rng.uniform(-2.0, 3.0, (depth, H, W, channels)).astype(np.float32)
    return v[..., 0] if channels == 1 else v


def coordinate_hitting(q, extent):
    """a float32 texture coordinate p with fl(fl(p * extent) - 0.5) == q exactly"""
    p0 = np.float32((q + 0.5) / extent)
    for p in (p0, np.nextafter(p0, np.float32(2)), np.nextafter(p0, np.float32(-2))):
        if np.float32(np.float32(p * np.float32(extent)) - np.float32(0.5)) == np.float32(q):
            return p
    raise AssertionError((q, extent))


def texture_points(depth=D):
    """cell centres; queries that land exactly on 0 and on extent - 1; just inside and just outside each of the six faces;
    z at -3.7, 0, 1 and 9.25 wrap periods and many periods away; points in the interior"""
    ext = (W, H, depth)
    pts = [((x + 0.5) / W, (y + 0.5) / H, (z + 0.5) / depth) for z in range(depth) for y in range(H) for x in range(W)]
    mid = [coordinate_hitting(0.5 * (e - 1), e) for e in ext]
    for a, e in enumerate(ext):
        for q in (0.0, float(e - 1)):
            p = list(mid)
            p[a] = coordinate_hitting(q, e)
            pts.append(tuple(p))
            for towards in (np.float32(2), np.float32(-2)):  # the nearest coordinates on either side that land elsewhere
                nudged = p[a]
                while np.float32(np.float32(nudged * np.float32(e)) - np.float32(0.5)) == np.float32(q):
                    nudged = np.nextafter(nudged, towards)
                p2 = list(p)
                p2[a] = nudged
                pts.append(tuple(p2))
        for face in (0.0, 1.0):  # the volume's own faces, half a cell beyond the first and last centres
            for off in (-1e-3, 1e-3):
                p = list(mid)
                p[a] = face + off
                pts.append(tuple(p))
    period = depth - 1
    for periods in (-3.7, 0.0, 1.0, 9.25, -250.5, 1000.0, 4001.125):
        pts.append((mid[0], mid[1], (periods * period + 0.5) / depth))
    rng = np.random.default_rng(5)
    pts += [tuple(p) for p in rng.uniform(-0.2, 1.2, (40, 3))]
    return np.array(pts, np.float32)


def posed_points(frame_kind, depth=D):
    """texture_points() carried back to map poses (frame 1) or world poses (frame 2) of FRAME, in float64 and rounded: the
    comparison is bit for bit whatever the points are"""
    tex = texture_points(depth).astype(np.float64)
    if frame_kind == 0:
        return tex.astype(np.float32)
    pose = tex * np.array([W, H, depth]) * FRAME[12:15].astype(np.float64)
    if frame_kind == 2:
        pose = pose @ FRAME[3:12].reshape(3, 3).astype(np.float64) + FRAME[0:3]  # R^T applied to rows, then the origin
    return pose.astype(np.float32)


def cases(depth=D):
    for ch, frame_kind, filt, address in itertools.product((1, 4), (0, 1, 2), (t3.LINEAR, t3.POINT), ADDRESSING):
        yield ch, frame_kind, filt, address


def test_points_cover_what_they_claim():
    pts = texture_points()
    q = [np.float32(np.float32(pts[:, a] * np.float32(e)) - np.float32(0.5)) for a, e in enumerate((W, H, D))]
    for a, e in enumerate((W, H, D)):
        assert (q[a] == 0).any() and (q[a] == e - 1).any() and (q[a] < 0).any() and (q[a] > e - 1).any()
        eps = np.float32(1e-6) * e
        assert ((q[a] > 0) & (q[a] < eps)).any() and ((q[a] < 0) & (q[a] > -eps)).any()
        assert ((q[a] > e - 1) & (q[a] < e - 1 + eps)).any() and ((q[a] < e - 1) & (q[a] > e - 1 - eps)).any()
    assert (q[2] > 1000 * (D - 1)).any() and (q[2] < -200 * (D - 1)).any()


@pytest.mark.parametrize("depth", [D, 2], ids=["depth5", "depth2"])
def test_shipped_helper_host_form_equals_restatement_bitwise(depth):
    """the __host__ form of the shipped helper — flags, selects, the closed-form wrap — against the restatement's early returns
    and loops, on every case the GPU test runs"""
    n = 0
    for ch, frame_kind, filt, address in cases(depth):
        data, pts = volume(depth, ch), posed_points(frame_kind, depth)
        kw = dict(frame_kind=frame_kind, address_mode=address, filter_mode=filt, border_color=BORDER_COLOR, frame=FRAME)
        want, got = t3.query(data, pts, **kw), t3.helper_query(data, pts, **kw)
        assert np.array_equal(bits(got), bits(want)), (ch, frame_kind, filt, address, np.flatnonzero((bits(got) != bits(want)).any(axis=1)))
        n += 1
    assert n == 2 * 3 * 2 * len(ADDRESSING)
    # border addressing returns the border colour exactly on 0 and keeps the value exactly on extent - 1
    data = volume(depth, 1)
    mid = [coordinate_hitting(0.5 * (e - 1), e) for e in (W, H, depth)]
    on0 = [coordinate_hitting(0.0, W), mid[1], mid[2]]
    on_last = [coordinate_hitting(W - 1.0, W), mid[1], mid[2]]
    got = t3.query(data, [on0, on_last], address_mode=(t3.BORDER,) * 3, border_color=BORDER_COLOR)[:, 0]
    assert got[0] == BORDER_COLOR[0] and got[1] != BORDER_COLOR[0]


def test_batch_form_equals_single_queries_on_the_host():
    data, pts = volume(D, 4), posed_points(2)[:48]
    for address in ADDRESSING:
        kw = dict(frame_kind=2, address_mode=address, border_color=BORDER_COLOR, frame=FRAME)
        single = t3.helper_query(data, pts, **kw)
        for batch in (1, 3, 4):
            assert np.array_equal(bits(t3.helper_query(data, pts, batch=batch, **kw)), bits(single)), (address, batch)


def test_wrap_closed_form_equals_the_loops():
    """wrapZ against the reference's two loops, in float32, for periods 1 .. 15 and coordinates up to thousands of periods away,
    multiples of the period and their float neighbours included"""
    L = t3.host()
    rng = np.random.default_rng(11)
    for period in (1, 2, 3, 4, 7, 15):
        P = np.float32(period)
        qs = np.concatenate([rng.uniform(-3000 * period, 3000 * period, 3000), rng.uniform(-2 * period, 3 * period, 500),
                             np.arange(-40, 41) * float(period), [-1e-30, 1e-30, -0.0, 0.0, -1e-7]]).astype(np.float32)
        qs = np.concatenate([qs, np.nextafter(qs, np.float32(1e9)), np.nextafter(qs, np.float32(-1e9))])
        for q in qs:
            want = np.float32(q)
            while want > P:
                want = np.float32(want - P)
            while want < 0:
                want = np.float32(want + P)
            got = np.float32(L.helper3d_wrap_z(float(q), float(P)))
            assert bits(got) == bits(want), (period, q, got, want)  # the sign of a zero included
        # at and beyond 2^20 periods, infinity included, the coordinate is taken as 0 (the loops would not end in useful time)
        for q in (np.float32(2.0 ** 20) * P, -np.float32(2.0 ** 20) * P, np.float32(1e30), np.float32(np.inf), np.float32(-np.inf)):
            assert bits(np.float32(L.helper3d_wrap_z(float(q), float(P)))) == bits(np.float32(0.0)), (period, q)
        q = np.nextafter(np.float32(2.0 ** 20) * P, np.float32(0))  # the last coordinate before that: still the loops' value
        assert np.float32(L.helper3d_wrap_z(float(q), float(P))) == np.float32(np.fmod(np.float64(q), period) or period)


def test_wrap_on_x_or_y_is_refused_on_the_host():
    L = t3.host()
    import ctypes as C
    why = C.create_string_buffer(200)
    for modes, depth, refused in (((2, 0, 0), 5, True), ((0, 2, 0), 5, True), ((0, 0, 2), 5, False), ((0, 0, 2), 1, True),
                                  ((1, 1, 2), 2, False), ((0, 3, 0), 5, True), ((0, 0, 0), 1, False)):
        assert bool(L.helper3d_modes_refused(np.array(modes, np.int32), depth, why, 200)) == refused, (modes, depth, why.value)


# ------------------------------------------------------------------ CPU: the host class -----------------------------------
def _layer(first, texels=200):
    i = np.arange(texels, dtype=np.float32) + np.float32(first)
    return np.ascontiguousarray(np.stack([i, i + 1, i + 2, i + 3], axis=1).reshape(-1))


def _dirty(L, depth):
    out = np.zeros(depth, np.int32)
    assert L.host3d_dirty(out, depth) == depth
    return out.tolist()


def _copy(L):
    log = np.zeros(64, np.int64)
    n = L.host3d_copy(log, 32)
    return [tuple(log[2 * i:2 * i + 2].tolist()) for i in range(n)]


def test_host_class_updates_and_dirty_layers():
    """UpdateTexture / UpdateTextureColumnMajor / UpdateTextureException / CopyDataToGPUSplitMiddle on ThreeDTextureHelperHost<1, 4>
    with a sink in host memory: row- and column-major updates give the same volume; an update marks its layer alone; a copy uploads the
    marked layers as contiguous slices and clears the marks; after setExtent every layer is marked"""
    L = t3.host()
    Wd, Hd, Dd, layer = 10, 20, 5, 10 * 20 * 4
    L.host3d_reset()
    assert L.host3d_set_extent(Wd, Hd, Dd) == 1 and L.host3d_set_extent(Wd, Hd, Dd) == 0
    assert _dirty(L, Dd) == [1] * Dd  # everything after setExtent
    assert _copy(L) == [(-1, Dd * layer), (0, Dd * layer)] and _dirty(L, Dd) == [0] * Dd
    # row-major layers: texel i of the volume holds i .. i + 3
    for z in range(Dd):
        assert L.host3d_update_layer(z, _layer(z * 200), layer, 0) == 0
        assert _dirty(L, Dd) == [1] * (z + 1) + [0] * (Dd - z - 1)
    row_major = np.zeros(Dd * layer, np.float32)
    assert L.host3d_values(row_major, row_major.size) == 0
    assert np.array_equal(row_major.reshape(-1, 4)[:, 0], np.arange(Dd * 200, dtype=np.float32))
    assert _copy(L) == [(0, Dd * layer)]
    # the same volume given column-major
    for z in range(Dd):
        texels = row_major.reshape(Dd, Hd, Wd, 4)[z]
        assert L.host3d_update_layer(z, np.ascontiguousarray(texels.transpose(1, 0, 2)).reshape(-1), layer, 1) == 0
    again = np.zeros_like(row_major)
    L.host3d_values(again, again.size)
    assert np.array_equal(again, row_major)
    _copy(L)
    # the split-middle sequence: odd layers, then even layers
    for z in (1, 3):
        assert L.host3d_update_layer(z, _layer((z + 5) * 200), layer, 0) == 0
    assert _dirty(L, Dd) == [0, 1, 0, 1, 0]
    assert _copy(L) == [(1 * layer, layer), (3 * layer, layer)] and _dirty(L, Dd) == [0] * Dd
    image, values = np.zeros(Dd * layer, np.float32), np.zeros(Dd * layer, np.float32)
    L.host3d_image(image, image.size), L.host3d_values(values, values.size)
    assert np.array_equal(image, values)
    out = np.zeros(4, np.float32)
    for zc, want in zip((0.1, 0.2, 0.3, 0.5, 0.6, 0.7), (0.0, 600, 1200, 400, 1000, 1600)):
        L.host3d_query_image(np.array([0, 0, zc], np.float32), out)
        assert_float_eq(out[0], want)
    for z in (0, 2, 4):
        L.host3d_update_layer(z, _layer((z + 10) * 200), layer, 0)
    assert _copy(L) == [(0, layer), (2 * layer, layer), (4 * layer, layer)]
    for zc, want in zip((0.1, 0.2, 0.3, 0.5, 0.6, 0.7), (2000.0, 1600, 1200, 2400, 2000, 1600)):
        L.host3d_query_image(np.array([0, 0, zc], np.float32), out)
        assert_float_eq(out[0], want)
    # neighbours travel as one slice, nothing changed travels not at all
    L.host3d_update_layer(2, _layer(1), layer, 0), L.host3d_update_layer(3, _layer(2), layer, 0)
    assert _copy(L) == [(2 * layer, 2 * layer)] and _copy(L) == []
    # exceptions: a buffer of the wrong size, a layer outside the extent, a zero depth, wrap on x
    assert L.host3d_update_layer(0, _layer(0, 30 * 40), 30 * 40 * 4, 0) == -1
    assert L.host3d_update_layer(Dd, _layer(0), layer, 0) == -1 and L.host3d_update_layer(-1, _layer(0), layer, 0) == -1
    assert L.host3d_update_volume(_layer(0), layer) == -1
    assert L.host3d_set_extent(Wd, Hd, 0) == -1 and L.host3d_set_extent(0, Hd, 2) == -1
    assert L.host3d_set_address_mode(0, 2) == -1 and L.host3d_set_address_mode(1, 2) == -1 and L.host3d_set_address_mode(2, 2) == 0
    assert _dirty(L, Dd) == [0] * Dd  # a refused call marks nothing
    # a new extent: all layers, a new allocation
    assert L.host3d_set_extent(Wd, Hd, 3) == 1 and _dirty(L, 3) == [1, 1, 1]
    assert _copy(L) == [(-1, 3 * layer), (0, 3 * layer)]


def test_host_program_under_sanitizers():
    """the stand-alone host program (its own main, no HIP call, nothing loaded into Python) built with
    -fsanitize=address,undefined walks the same scenarios in C++ and exits 0"""
    exe = t3.build_host_program()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "texture3d host checks passed" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------ GPU ------------------------------------------------
def _params(address, filt):
    return m.MppiTexture3dParams(origin=FRAME[0:3], rotations=FRAME[3:12], resolution=FRAME[12:15], address_mode=address,
                                 filter_mode=filt, border_color=BORDER_COLOR)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [D, 2], ids=["depth5", "depth2"])
def test_device_query_equals_restatement_bitwise(gpu, depth):
    """mppi_texture3d_query on a 4 x 3 x depth volume, 1 and 4 channels, the three frames, linear and point filtering, clamp and
    border on each axis independently and wrap on z, at texture_points(): bit for bit the restatement.  depth 2: min(floor, depth - 2)
    is always 0"""
    for ch, frame_kind, filt, address in cases(depth):
        data, pts = volume(depth, ch), posed_points(frame_kind, depth)
        want = t3.query(data, pts, frame_kind=frame_kind, address_mode=address, filter_mode=filt, border_color=BORDER_COLOR, frame=FRAME)
        got = m.texture3d_query(data, pts, frame_kind, _params(address, filt))
        assert np.array_equal(bits(got), bits(want)), (ch, frame_kind, filt, address, np.flatnonzero((bits(got) != bits(want)).any(axis=1)))


@pytest.mark.gpu
def test_device_batch_form_equals_single_queries(gpu):
    for ch in (1, 4):
        data, pts = volume(D, ch), posed_points(2)[:48]
        for address in ADDRESSING:
            single = m.texture3d_query(data, pts, 2, _params(address, t3.LINEAR))
            for batch in (1, 3, 4):
                got = m.texture3d_query(data, pts, 2, _params(address, t3.LINEAR), batch=batch)
                assert np.array_equal(bits(got), bits(single)), (ch, address, batch)


@pytest.mark.gpu
def test_device_query_refusals(gpu):
    """wrap on x or on y, wrap on one layer's worth of period, bad channels, extents below 2: MPPI_ERR_INVALID_ARG, nothing launched"""
    data, pts = volume(D, 1), texture_points()[:4]
    for address in ((t3.WRAP, 0, 0), (0, t3.WRAP, 0), (0, 0, 5)):
        with pytest.raises(m.MPPIError) as e:
            m.texture3d_query(data, pts, 0, _params(address, t3.LINEAR))
        assert e.value.status == m.MPPI_ERR_INVALID_ARG
    for bad in (np.zeros((5, 3, 4, 3), np.float32), np.zeros((1, 3, 4), np.float32), np.zeros((5, 3, 1), np.float32)):
        with pytest.raises(m.MPPIError) as e:
            m.texture3d_query(bad, pts, 0)
        assert e.value.status == m.MPPI_ERR_INVALID_ARG
    with pytest.raises(m.MPPIError) as e:
        m.texture3d_query(data, pts[:4], 0, batch=3)  # n is no multiple of the batch
    assert e.value.status == m.MPPI_ERR_INVALID_ARG


@pytest.mark.gpu
def test_layer_update_reaches_the_device_alone(gpu):
    """tests/probes/texture3d_layers_probe.hip: after updateTexture of layer 2 alone the copy is one slice of one layer into the same
    allocation; a query between layers 0 and 1 is unchanged, one between layers 2 and 3 changes, and both equal the host's values"""
    exe = nb.build_probe_program(m, "texture3d_layers_probe.hip")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "slices 1 first 2 count 1" in r.stdout and "same allocation 1" in r.stdout, r.stdout
    rows = re.findall(r"point (\d) before (\S+) after (\S+) host (\S+)", r.stdout)
    assert len(rows) == 2, r.stdout
    (_, b0, a0, h0), (_, b1, a1, h1) = rows
    assert float(b0) == float(a0) == float(h0) and float(b0) != 0
    assert float(b1) != float(a1) and float(a1) == float(h1)
