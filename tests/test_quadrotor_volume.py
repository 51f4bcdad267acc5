"""QuadrotorVolumeCost (QuadrotorQuadraticCost + a clearance volume read through ThreeDTextureHelper), registered as
"quadrotor_volume" by examples/quadrotor_model/quadrotor_volume_model.hip.  The cost is this project's own, not the reference's.

CPU: the volume term by hand at three positions of a 4 x 3 x 5 volume, on the restatement (tests/texture3d_oracle) and on the
shipped class's host form; the two against each other bit for bit; the parameter block; the registration.
GPU: every registered shape — the one-system ones fused and role-pipelined, the two-system one (64, 1, 2) as Tube MPPI fused,
pipelined and folded into a wave — and the rows-in-HBM forms against the restatement (costs 0 ulp, u* within 1e-5) with rollouts
that leave the volume through a face; two chained Philox iterations; what the "cost_volume" blob refuses."""
import ctypes as C

import numpy as np
import pytest

import mppi_generic_amd as m
import pyoracle as po
import quadrotor_oracle as qo
import texture3d_oracle as t3
from common import PHILOX_SEED, U_TOL, host_noise, make_engine, ulp_diff
from restate64 import bits

W, H, D = 4, 3, 5
CELL = 0.05  # metres per texel: the volume is 0.20 x 0.15 x 0.25 m


@pytest.fixture(scope="module")
def quadrotor_volume(lib):
    """built on its own through native_build and loaded with mppi_load_plugin, as tests/test_quadrotor.py does for "quadrotor" """
    return t3.load_model(m)


def x0_state():
    q0 = np.array([-0.93, -0.12, -0.15, 0.31])
    q0 = q0 / np.linalg.norm(q0)
    return np.concatenate([[0.1, 0.2, 0.8], [0.3, -0.1, 0.2], q0, [0.2, -0.4, 0.1]]).astype(np.float32)


def test_volume():
    """values in [-0.5, 1.5]: negative ones (max(0, v)), ones above the crash threshold of 0.9, and everything between"""
    return np.random.default_rng(3).uniform(-0.5, 1.5, (D, H, W)).astype(np.float32)


test_volume.__test__ = False


def volume_frame():
    """the start, (0.1, 0.2, 0.8), sits 3 cm under the volume's top face and in the middle of the other two axes: with 0.2 m/s of
    climb and thrust noise of 12 N some rollouts leave through the top face within T = 8 steps of 0.02 s, others stay inside"""
    return t3.frame15([0.1 - 0.10, 0.2 - 0.075, 0.8 - 0.195], np.eye(3), [CELL, CELL, CELL])


def volume_cfg(K=80, T=8, D_=1, num_iters=1):
    cost = m.QuadrotorVolumeCostParams()
    cost.s_goal[:] = [0.5, -0.3, 1.0, 0, 0, 0, 0.9689124, 0.0, 0.0, 0.24740396, 0, 0, 0]
    cost.x_coeff, cost.v_coeff, cost.w_coeff = 40.0, 15.0, 0.5
    cost.roll_coeff, cost.pitch_coeff, cost.yaw_coeff, cost.q_coeff = 15.0, 12.0, 9.0, 7.0
    cost.terminal_cost_coeff = 3.0
    cost.volume_coeff, cost.crash_threshold, cost.crash_coeff = 25.0, 0.9, 1000.0
    return dict(model="quadrotor_volume", K=K, T=T, D=D_, dt=0.02, lambda_=2.0, alpha=0.1, num_iters=num_iters,
                dyn=m.QuadrotorDynamicsParams(1.3), cost=cost, ranges=None, std_dev=[0.5, 0.5, 0.5, 12.0],
                control_cost_coeff=[2.0, 2.0, 2.0, 0.3], x0=x0_state(),
                blobs={"cost_volume_transform": volume_frame(), "cost_volume": test_volume()})


def make_volume_oracle(cfg):
    o = t3.QuadrotorVolumeOracle(cfg["K"], cfg["T"], cfg["D"], cfg["dt"], cfg["lambda_"], cfg["alpha"], cfg["num_iters"])
    o.set_dynamics_params(cfg["dyn"])
    o.set_cost_params(cfg["cost"])
    o.set_volume(cfg["blobs"]["cost_volume"], cfg["blobs"]["cost_volume_transform"])
    o.set_sampler(cfg["std_dev"], cfg["control_cost_coeff"], cfg.get("pure_pct", 0.01), cfg.get("decay", 1.0))
    return o


def nominal_control(T):
    """a non-zero mean: thrust around hover with steps near both ends of [0, 36], a constant roll rate"""
    u = np.zeros((T, 4), np.float32)
    u[:, 3] = 9.81
    u[1::3, 3] = 2.0
    u[2::3, 3] = 33.0
    u[:, 0] = 0.1
    return u


# ------------------------------------------------------------------ CPU -------------------------------------------------
def test_volume_term_by_hand():
    """a 4 x 3 x 5 volume whose value is 0.25 * layer, identity frame, one-metre cells: at height z the texel coordinate is
    z - 0.5 and v = 0.25 (z - 0.5), all exact in float32.  volume_coeff 8, crash_threshold 0.5, crash_coeff 1000.
      inside, z = 2.0:                 v = 0.375           term 3
      on the threshold, z = 2.5:       v = 0.5 (not above) term 4, no crash charge
      just above it, z = 3.0:          v = 0.625           term 5 + 1000
      outside through the x = 0 face:  border colour 0     term 0
    the quadratic part is the "quadrotor" restatement's on the same state"""
    values = np.broadcast_to((0.25 * np.arange(D, dtype=np.float32))[:, None, None], (D, H, W)).copy()
    p = m.QuadrotorVolumeCostParams()
    p.volume_coeff, p.crash_threshold, p.crash_coeff = 8.0, 0.5, 1000.0
    p.x_coeff = 3.0
    quad_p = m.QuadrotorQuadraticCostParams()
    quad_p.x_coeff = 3.0
    quad = qo.QuadrotorOracle(4, 3)
    quad.set_cost_params(quad_p)
    o = t3.QuadrotorVolumeOracle(4, 3)
    o.set_cost_params(p)
    o.set_volume(values, t3.IDENTITY_FRAME)
    hc = t3.HostCost()
    hc.set_cost_params(p)
    hc.set_volume(values, t3.IDENTITY_FRAME)
    assert t3.host().volume_cost_traits() == 7  # barrier-free, kernarg-viewable, border addressing on the three axes
    for pos, v, term in (((2.0, 1.5, 2.0), 0.375, 3.0), ((2.0, 1.5, 2.5), 0.5, 4.0), ((2.0, 1.5, 3.0), 0.625, 1005.0),
                         ((-1.0, 1.5, 2.0), 0.0, 0.0)):
        s = x0_state()
        s[0:3] = pos
        base = np.float32(quad.state_cost(s)[0])
        assert base > 0
        for got in (o.terms(s), hc.terms(s)):
            assert got[0] == np.float32(v) and got[1] == np.float32(term) and got[2] == base, (pos, got)
        want = np.float32(base + np.float32(term))
        assert np.float32(o.state_cost(s)[0]) == want and hc.state_cost(s) == want, pos
    # without a volume the term is 0; the terminal cost is the quadratic part's alone
    s = x0_state()
    s[0:3] = (2.0, 1.5, 3.0)
    p.terminal_cost_coeff = 2.0
    o.set_cost_params(p), hc.set_cost_params(p)
    base = np.float32(quad.state_cost(s)[0])
    assert hc.terminal_cost(s) == np.float32(2.0) * base == np.float32(o.terminal_cost(s))
    o.set_volume(None, None), hc.set_volume(None, None)
    assert o.terms(s)[1] == 0 and hc.terms(s)[1] == 0 and hc.state_cost(s) == base
    # a NaN position: MAX_COST_VALUE
    s[1] = np.nan
    assert hc.state_cost(s) == np.float32(1e16) and np.float32(o.state_cost(s)[0]) == np.float32(1e16)


def test_shipped_cost_host_form_equals_restatement_bitwise():
    cfg = volume_cfg()
    o = make_volume_oracle(cfg)
    hc = t3.HostCost()
    hc.set_cost_params(cfg["cost"])
    hc.set_volume(cfg["blobs"]["cost_volume"], cfg["blobs"]["cost_volume_transform"])
    rng = np.random.default_rng(17)
    inside = 0
    for _ in range(400):
        s = x0_state()
        s[0:3] += rng.uniform(-0.15, 0.15, 3).astype(np.float32)
        s[3:6] = rng.uniform(-1, 1, 3)
        a, b = o.terms(s), hc.terms(s)
        assert np.array_equal(bits(a), bits(b)), (s, a, b)
        assert bits(np.float32(o.state_cost(s)[0])) == bits(hc.state_cost(s))
        inside += a[0] != 0
    assert 20 < inside < 380  # positions on both sides of the faces


def test_parameter_block_and_registration(quadrotor_volume):
    block = m.QuadrotorVolumeCostParams()
    block.volume_coeff = -1
    t3.host().volume_cost_default_params(C.byref(block))
    assert bytes(block) == bytes(m.QuadrotorVolumeCostParams()) and C.sizeof(block) == 4 * 30
    assert bytes(block)[:4 * 27] == bytes(m.QuadrotorQuadraticCostParams())
    assert "quadrotor_volume" in m.list_models()
    qo.load_model(m)
    d, q = m.describe_model("quadrotor_volume"), m.describe_model("quadrotor")
    assert d["shapes"] == [(64, 1, 1), (64, 1, 2), (32, 4, 1), (16, 1, 1)] and d["pipeline"] and not d["rmppi"]
    assert m.describe_model("quadrotor_volume", m.MPPI_SAMPLER_COLORED) is None
    assert q is not None and d == q  # the shapes and the PIPELINE setting of "quadrotor", every capability bit included


# ------------------------------------------------------------------ GPU -------------------------------------------------
def forms():
    """every registered one-system shape as tests/kernel_forms.py chooses the forms, as tests/test_quadrotor.py lists them"""
    return [("fused64x1x1", (64, 1, 1), m.MPPI_KERNEL_FUSED), ("pipeline64x1x1", (64, 1, 1), m.MPPI_KERNEL_PIPELINE),
            ("fused32x4x1", (32, 4, 1), m.MPPI_KERNEL_FUSED), ("fused16x1x1", (16, 1, 1), m.MPPI_KERNEL_FUSED)]


FORMS = forms()


def test_forms_follow_kernel_forms(quadrotor_volume):
    from kernel_forms import pipeline_family
    d = m.describe_model("quadrotor_volume")
    want = []
    for sh in d["shapes"]:
        if sh[2] == 1:
            want.append(("fused%dx%dx%d" % sh, sh, m.MPPI_KERNEL_FUSED))
            if pipeline_family(d, sh):
                want.append(("pipeline%dx%dx%d" % sh, sh, m.MPPI_KERNEL_PIPELINE))
    assert want == FORMS
    # the one registered shape FORMS does not run, the two-system one, is test_tube's and test_tube_auto_fold_form's
    assert [sh for sh in d["shapes"] if sh[2] != 1] == [(64, 1, 2)] and pipeline_family(d, (64, 1, 2)) == "pipeline"


_REFERENCE = {}


def _reference_run(K, T):
    """one call of the CPU restatement, computed once per (K, T) and shared; asserts that the rollouts do what the test is for"""
    if (K, T) not in _REFERENCE:
        cfg = volume_cfg(K=K, T=T)
        o = make_volume_oracle(cfg)
        o.set_nominal_control(nominal_control(T))
        eps = host_noise(1, K, T, 4, seed=K + T)
        o.vanilla_compute_control(cfg["x0"], 1, eps)
        inside = o.inside(cfg["x0"], o.samples())
        assert inside.any() and (~inside).any(), inside.mean()          # samples inside and outside the volume
        assert (inside[:, 0] & ~inside[:, -1]).any()                    # rollouts that start inside and have left by the last step
        ref = dict(eps=eps, costs=o.costs().copy(), control=o.control().copy(), inside=inside)
        ref["costs"].setflags(write=False)
        _REFERENCE[(K, T)] = ref
    return _REFERENCE[(K, T)]


def test_rollouts_leave_the_volume():
    """the CPU half of the GPU test's premise: at K = 80 and at K = 16 some steps are inside and some outside; the volume term
    changes the costs"""
    for K in (80, 16):
        ref = _reference_run(K, 8)
        print("K = %d: %.0f %% of the rollout-steps inside the volume" % (K, 100 * ref["inside"].mean()))
    cfg = volume_cfg(K=16, T=8)
    o = make_volume_oracle(cfg)
    o.set_volume(None, None)
    o.set_nominal_control(nominal_control(8))
    o.vanilla_compute_control(cfg["x0"], 1, _reference_run(16, 8)["eps"])
    assert (o.costs() != _reference_run(16, 8)["costs"]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_every_shape_and_family_against_restatement(gpu, quadrotor_volume, form):
    """K = 80 (one full block of 64 and a partial one of 16) and K = 16, T = 8, injected noise around a non-zero mean: trajectory
    costs 0 ulp, u* within 1e-5"""
    name, shape, variant = form
    for K in (80, 16):
        ref = _reference_run(K, 8)
        cfg = volume_cfg(K=K, T=8)
        eng = make_engine(cfg, block_x=shape[0], block_y=shape[1], kernel_variant=variant, save_samples=True)
        try:
            eng.updateImportanceSampler(nominal_control(8))
            eng.injectNoise(ref["eps"])
            eng.computeControl(cfg["x0"], 1)
            info = eng.getLaunchInfo()
            assert info["block"] == shape and info["family"] == ("fused" if variant == m.MPPI_KERNEL_FUSED else "pipeline"), info
            dc = int(ulp_diff(eng.getSampledCostSeq(), ref["costs"]).max())
            du = float(np.abs(eng.getControlSeq() - ref["control"]).max())
            print("%s K=%d: costs %d ulp, u* %.3g" % (name, K, dc, du))
            assert dc == 0, "%s K=%d: costs differ by up to %d ulp" % (name, K, dc)
            assert du <= U_TOL, "%s K=%d: u* differs by %g" % (name, K, du)
        finally:
            eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [m.MPPI_KERNEL_FUSED, m.MPPI_KERNEL_PIPELINE], ids=["fused", "pipeline"])
def test_two_chained_philox_iterations(gpu, quadrotor_volume, variant):
    """K = 80, T = 9, two iterations with the in-kernel Philox noise: u* against the restatement on the same stream"""
    K, T = 80, 9
    cfg = volume_cfg(K=K, T=T, num_iters=2)
    eng = make_engine(cfg, block_x=64, block_y=1, kernel_variant=variant)
    try:
        eng.updateImportanceSampler(nominal_control(T))
        eng.setSeed(PHILOX_SEED)
        eng.computeControl(cfg["x0"], 1)
        o = make_volume_oracle(cfg)
        o.set_nominal_control(nominal_control(T))
        eps = np.stack([po.philox_normal(PHILOX_SEED, g, K, T, 4) for g in range(2)])
        o.vanilla_compute_control(cfg["x0"], 1, eps)
        du = float(np.abs(eng.getControlSeq() - o.control()).max())
        print("two Philox iterations: u* %.3g" % du)
        assert du <= U_TOL, du
    finally:
        eng.close()


# ------------------------------------------------------------------ GPU: the two-system shape and the other compiled forms --
_TUBE = {}


def _tube_reference():
    """Tube MPPI's first call on the restatement at K = 80, T = 8 (the nominal system starts at the actual state), shared"""
    if not _TUBE:
        cfg = volume_cfg(K=80, T=8, D_=2)
        eps = host_noise(1, 80, 8, 4, seed=5)
        o = make_volume_oracle(cfg)
        o.set_nominal_control(nominal_control(8))
        o.tube_compute_control(cfg["x0"], 1, eps)
        inside = o.inside(cfg["x0"], o.samples()[0])
        assert inside.any() and (~inside).any()
        _TUBE.update(cfg=cfg, eps=eps, costs=o.costs().copy(), control=o.control().copy(), nominal=o.nominal_control().copy())
    return _TUBE


def _check_tube(eng, ref):
    costs = eng.getSampledCostSeq()
    assert np.array_equal(bits(costs[0]), bits(costs[1]))  # both systems start at the same state
    dc = int(ulp_diff(costs, ref["costs"]).max())
    du = float(np.abs(eng.getControlSeq() - ref["control"]).max())
    dn = float(np.abs(eng.getNominalControlSeq() - ref["nominal"]).max())
    print("tube: costs %d ulp, u* %.3g, nominal u* %.3g" % (dc, du, dn))
    assert dc == 0 and du <= U_TOL and dn <= U_TOL, (dc, du, dn)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [m.MPPI_KERNEL_FUSED, m.MPPI_KERNEL_PIPELINE], ids=["fused", "pipeline"])
def test_tube(gpu, quadrotor_volume, variant):
    """Shape<64,1,2> — the form whose kernel keeps a by-value copy of the pointer-carrying cost next to two systems — at K = 80,
    T = 8: costs 0 ulp, u* and nominal u* within 1e-5 of the restatement's Tube computeControl"""
    ref = _tube_reference()
    eng = make_engine(ref["cfg"], block_x=64, block_y=1, kernel_variant=variant, save_samples=True)
    try:
        eng.updateImportanceSampler(nominal_control(8))
        eng.injectNoise(ref["eps"])
        eng.computeControl(ref["cfg"]["x0"], 1)
        info = eng.getLaunchInfo()
        assert info["block"] == (64, 1, 2) and info["family"] == ("fused" if variant == m.MPPI_KERNEL_FUSED else "pipeline"), info
        _check_tube(eng, ref)
    finally:
        eng.close()


@pytest.mark.gpu
def test_tube_auto_fold_form(gpu, quadrotor_volume):
    """a Tube controller created without a block shape folds the two systems into the lanes of a wave, (32,1,2)"""
    ref = _tube_reference()
    eng = make_engine(ref["cfg"], kernel_variant=m.MPPI_KERNEL_AUTO, save_samples=True)
    try:
        eng.updateImportanceSampler(nominal_control(8))
        eng.injectNoise(ref["eps"])
        eng.computeControl(ref["cfg"]["x0"], 1)
        info = eng.getLaunchInfo()
        assert info["family"] == "pipeline_fold" and info["block"] == (32, 1, 2), info
        _check_tube(eng, ref)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [m.MPPI_KERNEL_FUSED, m.MPPI_KERNEL_PIPELINE], ids=["fused", "pipeline"])
def test_rows_in_hbm_forms(gpu, quadrotor_volume, variant):
    """MPPI_AMD_ROWS_IN_HBM=1: the sample rows in HBM instead of LDS, the forms a long horizon runs, at K = 80, T = 8"""
    from kernel_forms import env_override
    ref = _reference_run(80, 8)
    cfg = volume_cfg(K=80, T=8)
    with env_override(MPPI_AMD_ROWS_IN_HBM="1"):
        eng = make_engine(cfg, block_x=64, block_y=1, kernel_variant=variant, save_samples=True)
    try:
        eng.updateImportanceSampler(nominal_control(8))
        eng.injectNoise(ref["eps"])
        eng.computeControl(cfg["x0"], 1)
        info = eng.getLaunchInfo()
        assert info["rows_in_hbm"] and info["block"] == (64, 1, 1), info
        assert int(ulp_diff(eng.getSampledCostSeq(), ref["costs"]).max()) == 0
        assert np.abs(eng.getControlSeq() - ref["control"]).max() <= U_TOL
    finally:
        eng.close()


def _raw_blob(eng, name, data, dims):
    data = np.ascontiguousarray(data, np.float32).reshape(-1)
    return eng._lib.mppi_set_model_blob(eng._h, name.encode(), data, data.size, (C.c_int * len(dims))(*dims), len(dims))


@pytest.mark.gpu
def test_cost_volume_blob_refusals(gpu, quadrotor_volume):
    """rank 2, a zero extent, three channels, a product that is not the count: MPPI_ERR_INVALID_ARG, the status "quadrotor_map"
    returns for a track map of the wrong rank; a good volume and its frame are taken"""
    cfg = volume_cfg(K=16, T=8)
    cfg["blobs"] = {}
    eng = make_engine(cfg)
    try:
        sixty = np.zeros(60, np.float32)
        for dims, text in (((15, 4), "rank 2"), ((5, 3, 4, 1, 1), "rank 5"), ((0, 3, 20), "positive"), ((5, 0, 12), "positive"),
                           ((5, 4, 1, 3), "1 or 4 channels"), ((5, 3, 1, 4), "reads 1 channel"), ((5, 3, 5), "count")):
            assert _raw_blob(eng, "cost_volume", sixty, dims) == m.MPPI_ERR_INVALID_ARG, dims
            assert text in eng._lib.mppi_last_error(eng._h).decode(), (dims, eng._lib.mppi_last_error(eng._h))
        assert _raw_blob(eng, "cost_volume_transform", sixty[:14], (14,)) == m.MPPI_ERR_INVALID_ARG
        assert _raw_blob(eng, "costmap", sixty, (15, 4)) != m.MPPI_OK  # the model has no 2-D map
        m.set_cost_volume(eng, test_volume(), origin=volume_frame()[0:3], resolution=volume_frame()[12:15])
        eng.computeControl(cfg["x0"], 1)
        assert np.isfinite(eng.getControlSeq()).all()
    finally:
        eng.close()
