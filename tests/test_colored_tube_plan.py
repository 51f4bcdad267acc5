"""Tube with the colored-noise sampler, before any device: the launch plan for a named sampler kind (planLaunch(cfg, sampler_kind,
...), mppi-generic_amd/csrc/launch_plan.hpp) against a stub model, the rule of mppi_set_independent_noise, and
mppi_create_with_sampler's checks that come before the device check.

tests/probes/launch_plan_sampler_probe.cpp is host-only C++ around the header, like tests/probes/launch_plan_probe.cpp (whose
cases run with each controller's own sampler and stay as they are).  The stub's LDS request is base + slots * T * c * 4 (+ ring
when pipelined); COL below has the capabilities of the double integrator's colored registration: the one- and the two-system
shape at 64 rollouts, a role pipeline and its fold, rows in HBM, two controls, and 8192 B that stand for the staging tiles of
the prologue GEMM (2 buffers x 4 k-steps x 4 time blocks x 64 lanes x 4 B).  Every expectation is derived by hand:

  Tube + colored never takes the pipelined or folded form, so AUTO and FUSED give the fused kernel on (64, 1, 2) with
  lds = 8192 + (64 * 2) * T * 2 * 4:  T = 8 -> 16384,  T = 6 -> 14336;  it fits up to T = 152 (163840 B = the limit);
  with the rows in HBM (overflow, or MPPI_AMD_ROWS_IN_HBM) only the staging tiles remain: 8192.
  The same stub with the Gaussian or the NLN sampler folds as before: (32, 1, 2), 8192 + 4096 + 64 * 8 * 2 * 4 = 16384.
"""
import ctypes as C
import subprocess

import pytest

import mppi_generic_amd as m
import native_build as nb
from mppi_generic_amd import capi


VANILLA, TUBE, ROBUST, COLORED = 0, 1, 2, 3
AUTO, FUSED, PIPELINE = 0, 1, 2
GAUSSIAN, COLORED_NOISE, NLN = m.MPPI_SAMPLER_GAUSSIAN, m.MPPI_SAMPLER_COLORED, m.MPPI_SAMPLER_NLN
SHAPE, OVERFLOW, UNSUPPORTED, INVALID = (m.MPPI_ERR_LAUNCH_SHAPE, m.MPPI_ERR_LDS_OVERFLOW, m.MPPI_ERR_UNSUPPORTED,
                                         m.MPPI_ERR_INVALID_ARG)

SAMPLER_TEXT = ("mppi_create: the Vanilla, Tube and Robust controllers take MPPI_SAMPLER_GAUSSIAN or MPPI_SAMPLER_NLN, "
                "MPPI_CONTROLLER_COLORED takes MPPI_SAMPLER_COLORED only")
ROBUST_COLORED_TEXT = ("mppi_create: Robust MPPI with MPPI_SAMPLER_COLORED is not available: its candidate evaluation draws single "
                       "samples by index (random access), the colored-noise rows come out of a block-wide GEMM prologue and have no "
                       "such draw")
TUBE_PIPELINE_TEXT = ("mppi_create: the pipeline variant has no form for the Tube controller with MPPI_SAMPLER_COLORED; it runs the "
                      "fused kernel (MPPI_KERNEL_AUTO or MPPI_KERNEL_FUSED)")
INDEP_TUBE_TEXT = ("independent noise per distribution: the colored-noise sampler draws one spectrum per rollout for both systems "
                   "of a Tube handle; no per-system spectrum stream is assigned")
INDEP_COLORED_TEXT = "independent noise per distribution: the colored-noise sampler has one distribution"


def overflow_text(n):
    return ("mppi_create: rollout kernel needs %d B of LDS per block (max 163840) — the sample rows of a block live in LDS and "
            "this sampler / controller / kernel variant has no rows-in-HBM form; shorten the horizon or register a block shape "
            "with fewer rollouts" % n)


COL = "shapes=64x1x1,64x1x2 pipeline=1 fold=1 hbm=1 c=2 base=8192 ring=4096"
COL_NO_HBM = "shapes=64x1x1,64x1x2 pipeline=1 fold=1 c=2 base=8192 ring=4096"
# a registration that lists more two-system shapes, as the templated controllers' RolloutShapes does
COL_TPL = "shapes=64x1x1,64x1x2,32x1x1,32x1x2,64x4x1,64x4x2 pipeline=1 fold=1 hbm=1 c=2 base=8192 ring=4096"
COL_TPL_NO_HBM = "shapes=64x1x1,64x1x2,32x1x1,32x1x2,64x4x1,64x4x2 pipeline=1 fold=1 c=2 base=8192 ring=4096"


def only_64x1x2_text(bx, by):
    return ("mppi_create: the Tube controller with MPPI_SAMPLER_COLORED runs block shape (64,1,2) only — the one shape whose "
            "prologue has been held to the oracle with two systems; (%d,%d,2) was asked for" % (bx, by))


def ok(D, bx, by, pipeline=0, hbm=0, lds=0):
    return "ok %d %d %d %d %d 0 %d %d rows=null" % (D, bx, by, D, pipeline, hbm, lds)


def refused(status, text):
    return "refused %d rows=null %s" % (status, text)


def req(ctl, sampler, T=8, variant=AUTO, bx=0, by=0, forced=0):
    return "ctl=%d sampler=%d T=%d variant=%d bx=%d by=%d forced=%d" % (ctl, sampler, T, variant, bx, by, forced)


# (id, model, request, expected line)
TABLE = [
    # --- accepted: D = 2, block (64, 1, 2), the fused kernel, rows of 64 x 2 slots + the staging tiles
    ("tube-colored-T8", COL, req(TUBE, COLORED_NOISE, T=8), ok(2, 64, 1, lds=16384)),
    ("tube-colored-T6", COL, req(TUBE, COLORED_NOISE, T=6), ok(2, 64, 1, lds=14336)),
    ("tube-colored-fused-request", COL, req(TUBE, COLORED_NOISE, variant=FUSED), ok(2, 64, 1, lds=16384)),
    ("tube-colored-explicit-64x1", COL, req(TUBE, COLORED_NOISE, bx=64, by=1), ok(2, 64, 1, lds=16384)),
    ("tube-colored-last-fitting-T", COL_NO_HBM, req(TUBE, COLORED_NOISE, T=152), ok(2, 64, 1, lds=163840)),
    # --- no pipelined or folded form: the request is refused, the fold's shape is not instantiated
    ("tube-colored-pipeline-refused", COL, req(TUBE, COLORED_NOISE, variant=PIPELINE), refused(SHAPE, TUBE_PIPELINE_TEXT)),
    ("tube-colored-pipeline-refused-on-64x1", COL, req(TUBE, COLORED_NOISE, variant=PIPELINE, bx=64, by=1),
     refused(SHAPE, TUBE_PIPELINE_TEXT)),
    ("tube-colored-fold-shape-refused", COL, req(TUBE, COLORED_NOISE, bx=32, by=1),
     refused(SHAPE, "mppi_create: block shape (32,1,2) is not instantiated for model 'stub'")),
    ("tube-colored-no-two-system-shape", "shapes=64x1x1 pipeline=1 fold=1 hbm=1 c=2 base=8192 ring=4096", req(TUBE, COLORED_NOISE),
     refused(SHAPE, "mppi_create: block shape (64,1,2) is not instantiated for model 'stub'")),
    # --- (64, 1, 2) only, whatever else the registration lists: no other shape has run with two systems' rows from the prologue
    ("tube-colored-many-shapes-default", COL_TPL, req(TUBE, COLORED_NOISE), ok(2, 64, 1, lds=16384)),
    ("tube-colored-32x1x2-refused", COL_TPL, req(TUBE, COLORED_NOISE, bx=32, by=1), refused(SHAPE, only_64x1x2_text(32, 1))),
    ("tube-colored-64x4x2-refused", COL_TPL, req(TUBE, COLORED_NOISE, bx=64, by=4), refused(SHAPE, only_64x1x2_text(64, 4))),
    ("tube-colored-32x1x2-refused-fused-request", COL_TPL, req(TUBE, COLORED_NOISE, variant=FUSED, bx=32, by=1),
     refused(SHAPE, only_64x1x2_text(32, 1))),
    ("tube-colored-overflow-takes-no-smaller-shape", COL_TPL_NO_HBM, req(TUBE, COLORED_NOISE, T=153),
     refused(OVERFLOW, overflow_text(8192 + 1024 * 153))),
    ("tube-gaussian-keeps-32x1x2-fused", COL_TPL, req(TUBE, GAUSSIAN, variant=FUSED, bx=32, by=1), ok(2, 32, 1, lds=8192 + 512 * 8)),
    # --- long horizons: the rows in HBM where the sampler has them, else the overflow refusal
    ("tube-colored-rows-in-hbm-on-overflow", COL, req(TUBE, COLORED_NOISE, T=700), ok(2, 64, 1, hbm=1, lds=8192)),
    ("tube-colored-rows-in-hbm-forced", COL, req(TUBE, COLORED_NOISE, forced=1), ok(2, 64, 1, hbm=1, lds=8192)),
    ("tube-colored-overflow-refused", COL_NO_HBM, req(TUBE, COLORED_NOISE, T=153), refused(OVERFLOW, overflow_text(8192 + 1024 * 153))),
    ("tube-colored-overflow-refused-long", COL_NO_HBM, req(TUBE, COLORED_NOISE, T=700), refused(OVERFLOW, overflow_text(8192 + 1024 * 700))),
    ("tube-colored-hbm-form-overflows-too", "shapes=64x1x1,64x1x2 hbm=1 c=2 base=170000", req(TUBE, COLORED_NOISE),
     refused(OVERFLOW, overflow_text(170000))),
    # --- the sampler rule
    ("robust-colored-unsupported", COL, req(ROBUST, COLORED_NOISE), refused(UNSUPPORTED, ROBUST_COLORED_TEXT)),
    ("robust-colored-unsupported-before-the-shape", COL, req(ROBUST, COLORED_NOISE, bx=16), refused(UNSUPPORTED, ROBUST_COLORED_TEXT)),
    ("vanilla-colored-invalid", COL, req(VANILLA, COLORED_NOISE), refused(INVALID, SAMPLER_TEXT)),
    ("colored-gaussian-invalid", COL, req(COLORED, GAUSSIAN), refused(INVALID, SAMPLER_TEXT)),
    ("colored-nln-invalid", COL, req(COLORED, NLN), refused(INVALID, SAMPLER_TEXT)),
    ("tube-unknown-sampler-invalid", COL, req(TUBE, 9), refused(INVALID, SAMPLER_TEXT)),
    ("unknown-controller-with-colored-invalid", COL, req(7, COLORED_NOISE), refused(INVALID, SAMPLER_TEXT)),
    ("unknown-controller-reported-by-the-plan", COL, req(7, GAUSSIAN),
     refused(UNSUPPORTED, "mppi_create: controller kind not available in this build")),
    # --- every other combination as before: the same stub folds with the Gaussian and the NLN sampler, pipelines for Colored
    ("tube-gaussian-still-folds", COL, req(TUBE, GAUSSIAN), ok(2, 32, 1, pipeline=1, lds=16384)),
    ("tube-nln-still-folds", COL, req(TUBE, NLN), ok(2, 32, 1, pipeline=1, lds=16384)),
    ("tube-gaussian-pipeline-request", COL, req(TUBE, GAUSSIAN, variant=PIPELINE, bx=64, by=1),
     ok(2, 64, 1, pipeline=1, lds=8192 + 4096 + 128 * 8 * 2 * 4)),
    ("colored-controller-still-pipelines", COL, req(COLORED, COLORED_NOISE), ok(1, 64, 1, pipeline=1, lds=8192 + 4096 + 64 * 8 * 2 * 4)),
]

# (id, controller, sampler, expected line)
INDEP = [
    ("tube-colored", TUBE, COLORED_NOISE, "indep-refused %d %s" % (UNSUPPORTED, INDEP_TUBE_TEXT)),
    ("colored-controller", COLORED, COLORED_NOISE, "indep-refused %d %s" % (UNSUPPORTED, INDEP_COLORED_TEXT)),
    ("tube-gaussian", TUBE, GAUSSIAN, "indep-ok"),
    ("tube-nln", TUBE, NLN, "indep-ok"),
    ("robust-gaussian", ROBUST, GAUSSIAN, "indep-ok"),
    ("vanilla-gaussian", VANILLA, GAUSSIAN, "indep-ok"),
]


def _build(sanitize):
    return nb.build_plan_probe("launch_plan_sampler_probe", sanitize)


def _run(exe):
    text = "".join("%s %s\n" % (model, request) for _, model, request, _ in TABLE)
    text += "".join("indep=1 ctl=%d sampler=%d\n" % (ctl, sampler) for _, ctl, sampler, _ in INDEP)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(TABLE) + len(INDEP), r.stdout
    return lines


@pytest.fixture(scope="module")
def answers():
    lines = _run(_build(sanitize=False))
    return dict(zip([t[0] for t in TABLE] + ["indep:" + t[0] for t in INDEP], lines))


def test_case_ids_are_unique():
    assert len({t[0] for t in TABLE}) == len(TABLE) and len({t[0] for t in INDEP}) == len(INDEP)


@pytest.mark.parametrize("case", TABLE, ids=[t[0] for t in TABLE])
def test_plan_for_a_named_sampler(answers, case):
    """the plan, or the status and text — and the stub's row pointer is null again after the call"""
    tag, _, _, want = case
    assert answers[tag] == want
    assert " rows=null" in answers[tag]


@pytest.mark.parametrize("case", INDEP, ids=[t[0] for t in INDEP])
def test_independent_noise_rule(answers, case):
    tag, _, _, want = case
    assert answers["indep:" + tag] == want


def test_sampler_probe_is_clean_under_address_and_ub_sanitizers():
    """the same stand-alone program built with -fsanitize=address,undefined, once over both tables: same lines, no report"""
    assert _run(_build(sanitize=True)) == [t[3] for t in TABLE] + [t[3] for t in INDEP]


# ------------------------------------------------------------------ mppi_create_with_sampler before the device check ---------
def _cfg(**kw):
    cfg = capi.MppiConfig(model=b"double_integrator", controller=TUBE, num_rollouts=64, num_timesteps=8, dt=0.02, lambda_=1.0,
                          alpha=0.0, num_iters=1, seed=1, noise_source=0, block_x=0, block_y=0, device=0, stream=None, rank=0,
                          world_size=1, save_samples=0, kernel_variant=AUTO, force_exchange=0)
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _create(lib, cfg, sampler):
    out = capi.H(0x1234)
    st = lib.mppi_create_with_sampler(C.byref(cfg), sampler, C.byref(out))
    text = lib.mppi_last_error(None).decode() if st != m.MPPI_OK else ""
    if st == m.MPPI_OK:
        lib.mppi_destroy(out)
    else:
        assert out.value is None
    return st, text


def test_tube_with_the_colored_sampler_passes_the_argument_checks(lib):
    """accepted: with a device the handle is created, without one the refusal is the device's, not the sampler rule's"""
    st, text = _create(lib, _cfg(), COLORED_NOISE)
    if lib.mppi_device_count() > 0:
        assert st == m.MPPI_OK, text
    else:
        assert st == m.MPPI_ERR_NO_DEVICE, (st, text)
    # ... on both in-tree models, and the sizes are checked once the sampler rule has passed
    st, text = _create(lib, _cfg(model=b"cartpole", num_rollouts=0), COLORED_NOISE)
    assert (st, text) == (INVALID, "mppi_create: num_rollouts, num_timesteps, dt, lambda, num_iters must be > 0")


def test_robust_with_the_colored_sampler_is_unsupported_before_the_device(lib):
    st, text = _create(lib, _cfg(controller=ROBUST), COLORED_NOISE)
    assert (st, text) == (UNSUPPORTED, ROBUST_COLORED_TEXT)
    # before the sizes too, like every sampler mismatch
    st, text = _create(lib, _cfg(controller=ROBUST, num_rollouts=0), COLORED_NOISE)
    assert (st, text) == (UNSUPPORTED, ROBUST_COLORED_TEXT)


def test_other_sampler_mismatches_keep_status_and_text(lib):
    for cfg, sampler in ((_cfg(controller=VANILLA), COLORED_NOISE), (_cfg(controller=COLORED), GAUSSIAN), (_cfg(), 9)):
        assert _create(lib, cfg, sampler) == (INVALID, SAMPLER_TEXT)


def test_mppi_create_keeps_tube_on_the_gaussian_sampler(lib):
    """mppi_create(cfg) is mppi_create_with_sampler(cfg, GAUSSIAN) for Tube: same outcome with or without a device"""
    out = capi.H()
    cfg = _cfg()
    st = lib.mppi_create(C.byref(cfg), C.byref(out))
    if st == m.MPPI_OK:
        assert lib.mppi_get_sampler_kind(out) == GAUSSIAN
        lib.mppi_destroy(out)
    else:
        assert st == m.MPPI_ERR_NO_DEVICE


def test_the_two_system_kernels_are_a_registration_of_their_own(lib):
    """MPPI_CONTROLLER_COLORED's registrations stay one-system; what Tube runs is listed under MPPI_SAMPLER_COLORED_TUBE: the fused
    (64, 1, 2) and no role-pipelined form.  The key registers and describes, it creates nothing"""
    for name in ("double_integrator", "cartpole"):
        one = m.describe_model(name, COLORED_NOISE)
        assert one["shapes"] and all(s[2] == 1 for s in one["shapes"]), (name, one["shapes"])
        two = m.describe_model(name, m.MPPI_SAMPLER_COLORED_TUBE)
        assert two["shapes"] == [(64, 1, 2)] and two["rows_in_hbm"], (name, two)
        assert not two["pipeline"] and not two["pipeline_fold"] and not two["rmppi"] and not two["streamed_merge"], (name, two)
    assert m.describe_model("autorally_nn", m.MPPI_SAMPLER_COLORED_TUBE) is None
    for cfg in (_cfg(), _cfg(controller=COLORED), _cfg(controller=VANILLA)):
        assert _create(lib, cfg, m.MPPI_SAMPLER_COLORED_TUBE) == (INVALID, SAMPLER_TEXT)
