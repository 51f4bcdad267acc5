"""mppi-generic_amd/csrc/launch_plan.hpp: planLaunch — which rollout kernel a handle runs — against a stub model, on the CPU.

tests/probes/launch_plan_probe.cpp is host-only C++ around the header; its stub model's capabilities and its linear LDS formula
(base + slots * T * c * 4 (+ ring when pipelined), the row term dropped while the row pointer is set) come from the case line.
Every expectation below was derived by hand from mppi_create_with_sampler as it stood before the plan was split out of it
(engine_core.hip at commit 5b0af06); the case id names the lines.  160 KiB = 163840 B is the LDS limit.

The second half holds mppi_create's checks that come before the device check to status and exact text, through the real library.
"""
import ctypes as C
import subprocess

import pytest

import mppi_generic_amd as m
import native_build as nb
from mppi_generic_amd import capi


VANILLA, TUBE, ROBUST, COLORED = 0, 1, 2, 3
AUTO, FUSED, PIPELINE = 0, 1, 2
SHAPE, OVERFLOW, UNSUPPORTED = m.MPPI_ERR_LAUNCH_SHAPE, m.MPPI_ERR_LDS_OVERFLOW, m.MPPI_ERR_UNSUPPORTED

ROBUST_SHAPE_TEXT = "mppi_create: Robust MPPI runs with block shape (64, 1, 2) or (32, 1, 2)"
ROBUST_PIPELINE_TEXT = ("mppi_create: the pipelined Robust MPPI kernel needs a model registered for it (replicated-lane MFMA / "
                        "four-lane dynamics, or a one-lane model registered with PIPELINE), the Gaussian sampler and block_x 0 or 64")
PIPELINE_TEXT = ("mppi_create: the pipeline variant needs a model registered for it and block shape (64, 1), or (64, REP, 1) "
                 "for replicated-lane (MFMA) dynamics")


def overflow_text(n):
    return ("mppi_create: rollout kernel needs %d B of LDS per block (max 163840) — the sample rows of a block live in LDS and "
            "this sampler / controller / kernel variant has no rows-in-HBM form; shorten the horizon or register a block shape "
            "with fewer rollouts" % n)


# stub models (c = 1: a row is T * 4 bytes per slot; 64 slots overflow above T = 640 - base / 256)
ROB = "shapes=64x1x1 rmppi=1 base=1024"                  # rmppiSharedBytes: 1024 + bx * 2 * T * 4
ONE = "shapes=64x1x1 base=1024"                          # fused only: 1024 + 64 * T * 4
PIPE = "shapes=64x1x1,16x4x1 pipeline=1 base=1024 ring=4096"
FOLD = "shapes=64x1x1,64x1x2 pipeline=1 fold=1 base=1024 ring=4096"
BZ1 = "default=64x4 shapes=64x4x1,16x1x2,32x4x2 base=1024"    # the default (64, 4) exists for one system only
MANY = "shapes=64x1x1,32x2x1,32x1x1,16x4x1 base=1024"


def ok(D, bx, by, pipeline=0, rm=0, hbm=0, lds=0):
    return "ok %d %d %d %d %d %d %d %d rows=null" % (D, bx, by, D, pipeline, rm, hbm, lds)


def refused(status, text):
    return "refused %d rows=null %s" % (status, text)


def req(ctl, T=8, variant=AUTO, bx=0, by=0, forced=0):
    return "ctl=%d T=%d variant=%d bx=%d by=%d forced=%d" % (ctl, T, variant, bx, by, forced)


# (id, model, request, expected line)
TABLE = [
    # --- the controller kind (L322-334)
    ("L328-robust-not-instantiated", ONE, req(ROBUST), refused(UNSUPPORTED, "mppi_create: model 'stub' is not instantiated for Robust MPPI")),
    ("L333-unknown-controller", ONE, req(7), refused(UNSUPPORTED, "mppi_create: controller kind not available in this build")),
    # --- Robust MPPI's block (L343-351): 1024 + 512 T fits up to T = 318, 1024 + 256 T up to T = 636
    ("L345-robust-bx16-refused", ROB, req(ROBUST, bx=16), refused(SHAPE, ROBUST_SHAPE_TEXT)),
    ("L345-robust-by4-refused", ROB, req(ROBUST, by=4), refused(SHAPE, ROBUST_SHAPE_TEXT)),
    ("L347-robust-64-at-the-last-fitting-T", ROB, req(ROBUST, T=318), ok(2, 64, 1, lds=163840)),
    ("L349-robust-64-to-32-on-overflow", ROB, req(ROBUST, T=319), ok(2, 32, 1, lds=1024 + 256 * 319)),
    ("L349-robust-explicit-64-is-not-halved", ROB, req(ROBUST, T=319, bx=64), refused(OVERFLOW, overflow_text(1024 + 512 * 319))),
    # --- Robust MPPI's pipelined form (L352-371); with it the LDS check is on rmppiSharedBytes(64) with the rows in HBM (L416)
    ("L359-robust-pipelined-chosen", ROB + " hbm=1 rmpipe=100000", req(ROBUST), ok(2, 64, 1, rm=1, hbm=1, lds=1024)),
    ("L363-robust-pipelined-undoes-the-32", ROB + " hbm=1 rmpipe=100000", req(ROBUST, T=319), ok(2, 64, 1, rm=1, hbm=1, lds=1024)),
    ("L352-robust-fused-request-skips-it", ROB + " hbm=1 rmpipe=100000", req(ROBUST, variant=FUSED), ok(2, 64, 1, lds=1024 + 512 * 8)),
    ("L353-robust-bx32-skips-it", ROB + " hbm=1 rmpipe=100000", req(ROBUST, bx=32), ok(2, 32, 1, lds=1024 + 256 * 8)),
    ("L359-robust-rings-do-not-fit", ROB + " hbm=1 rmpipe=163841", req(ROBUST), ok(2, 64, 1, lds=1024 + 512 * 8)),
    ("L368-robust-pipeline-refused", ROB + " hbm=1", req(ROBUST, variant=PIPELINE), refused(SHAPE, ROBUST_PIPELINE_TEXT)),
    ("L368-robust-pipeline-bx32-refused", ROB + " hbm=1 rmpipe=100000", req(ROBUST, variant=PIPELINE, bx=32), refused(SHAPE, ROBUST_PIPELINE_TEXT)),
    ("L345-before-L368-robust-pipeline-and-bx16", ROB + " hbm=1 rmpipe=100000", req(ROBUST, variant=PIPELINE, bx=16), refused(SHAPE, ROBUST_SHAPE_TEXT)),
    ("L368-before-L441-forced-hbm-with-pipeline-on-robust", ROB + " hbm=1", req(ROBUST, variant=PIPELINE, forced=1), refused(SHAPE, ROBUST_PIPELINE_TEXT)),
    # --- Robust MPPI's rows in HBM (L441-453)
    ("L446-robust-rows-in-hbm-at-64", ROB + " hbm=1", req(ROBUST, T=637), ok(2, 64, 1, hbm=1, lds=1024)),
    ("L447-robust-forced-keeps-64", ROB + " hbm=1", req(ROBUST, forced=1), ok(2, 64, 1, hbm=1, lds=1024)),
    ("L447-robust-forced-keeps-the-32", ROB + " hbm=1", req(ROBUST, T=319, forced=1), ok(2, 32, 1, hbm=1, lds=1024)),
    ("L441-robust-no-hbm-form-overflows", ROB, req(ROBUST, T=637), refused(OVERFLOW, overflow_text(1024 + 256 * 637))),
    # --- the Tube fold (L373-379): 1024 + 4096 + 64 * 8 * 4
    ("L373-tube-auto-fold", FOLD, req(TUBE), ok(2, 32, 1, pipeline=1, lds=7168)),
    ("L374-tube-fused-request-does-not-fold", FOLD, req(TUBE, variant=FUSED), ok(2, 64, 1, lds=1024 + 128 * 8 * 4)),
    ("L373-explicit-block_x-beats-the-fold", FOLD, req(TUBE, bx=64), ok(2, 64, 1, pipeline=1, lds=1024 + 4096 + 128 * 8 * 4)),
    ("L373-block_y-alone-skips-the-fold", FOLD, req(TUBE, by=1), ok(2, 64, 1, pipeline=1, lds=1024 + 4096 + 128 * 8 * 4)),
    # --- the default shape for bz (L383-401)
    ("L393-default-missing-for-bz-same-by", BZ1, req(TUBE), ok(2, 32, 4, lds=1024 + 64 * 8 * 4)),
    ("L393-default-missing-for-bz-first-listed", "default=64x4 shapes=64x4x1,16x1x2,32x2x2 base=1024", req(TUBE), ok(2, 16, 1, lds=1024 + 32 * 8 * 4)),
    # --- refusals of a shape (L403-414)
    ("L403-uninstantiated-shape-refused", PIPE, req(VANILLA, bx=16, by=1), refused(SHAPE, "mppi_create: block shape (16,1,1) is not instantiated for model 'stub'")),
    ("L403-nothing-registered-for-bz", ONE, req(TUBE), refused(SHAPE, "mppi_create: block shape (64,1,2) is not instantiated for model 'stub'")),
    ("L411-pipeline-on-unpipelined-shape-refused", PIPE, req(VANILLA, variant=PIPELINE, bx=16, by=4), refused(SHAPE, PIPELINE_TEXT)),
    ("L410-replicated-lane-shape-pipelines", "shapes=64x4x1,64x1x1 rep=64x4x1 piperep=1 base=1024 ring=4096", req(VANILLA, variant=PIPELINE, bx=64, by=4), ok(1, 64, 4, pipeline=1, lds=1024 + 4096 + 64 * 8 * 4)),
    # --- the pipelined kernel's rows in HBM (L421-434): 1024 + 4096 + 256 T overflows above T = 620
    ("L415-pipeline-by-default", PIPE, req(VANILLA), ok(1, 64, 1, pipeline=1, lds=1024 + 4096 + 64 * 8 * 4)),
    ("L421-pipeline-rows-in-hbm-on-overflow", PIPE + " hbm=1", req(VANILLA, T=700), ok(1, 64, 1, pipeline=1, hbm=1, lds=5120)),
    ("L421-pipeline-rows-in-hbm-on-hbm_forced", PIPE + " hbm=1", req(VANILLA, forced=1), ok(1, 64, 1, pipeline=1, hbm=1, lds=5120)),
    ("L421-pipeline-request-rows-in-hbm", PIPE + " hbm=1", req(VANILLA, T=700, variant=PIPELINE), ok(1, 64, 1, pipeline=1, hbm=1, lds=5120)),
    # --- AUTO falls back to the fused kernel (L435-439): T = 630: 166400 pipelined, 162304 fused
    ("L435-auto-falls-back-to-fused", PIPE, req(VANILLA, T=630), ok(1, 64, 1, lds=162304)),
    ("L435-pipeline-request-does-not-fall-back", PIPE, req(VANILLA, T=630, variant=PIPELINE), refused(OVERFLOW, overflow_text(166400))),
    # --- the fused kernel's rows in HBM on the default shape (L454-475)
    ("L454-fused-rows-in-hbm-on-the-default-shape", ONE + " hbm=1", req(VANILLA, T=700), ok(1, 64, 1, hbm=1, lds=1024)),
    ("L454-fused-rows-in-hbm-on-hbm_forced", ONE + " hbm=1", req(VANILLA, variant=FUSED, forced=1), ok(1, 64, 1, hbm=1, lds=1024)),
    ("L454-hbm_forced-without-an-hbm-form-is-ignored", ONE, req(VANILLA, forced=1), ok(1, 64, 1, lds=1024 + 64 * 8 * 4)),
    ("L427-then-L454-ring-overflows-alone-fused-rows-in-hbm", "shapes=64x1x1 pipeline=1 hbm=1 base=1024 ring=163000", req(VANILLA, T=700), ok(1, 64, 1, hbm=1, lds=1024)),
    ("L465-then-L476-default-undone-and-unregistered-shape-search", BZ1 + " hbm=1", req(TUBE, T=700), ok(2, 16, 1, lds=1024 + 32 * 700 * 4)),
    ("L469-hbm-form-overflows-too-its-figure-is-reported", "shapes=64x1x1 hbm=1 base=170000", req(VANILLA), refused(OVERFLOW, overflow_text(170000))),
    # --- no rows-in-HBM form: the largest registered shape that fits (L476-500), else the refusal (L501-505)
    ("L476-largest-fitting-shape-first-listed-among-equals", MANY, req(VANILLA, T=700), ok(1, 32, 2, lds=1024 + 32 * 700 * 4)),
    ("L476-explicit-shape-is-not-searched", MANY, req(VANILLA, T=700, bx=64, by=1), refused(OVERFLOW, overflow_text(1024 + 64 * 700 * 4))),
    ("L501-lds-overflow-refused", ONE, req(VANILLA, T=700), refused(OVERFLOW, overflow_text(180224))),
]


def _build(sanitize):
    return nb.build_plan_probe("launch_plan_probe", sanitize)


def _run(exe):
    text = "".join("%s %s\n" % (model, request) for _, model, request, _ in TABLE)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(TABLE), r.stdout
    return lines


@pytest.fixture(scope="module")
def plans():
    return dict(zip((t[0] for t in TABLE), _run(_build(sanitize=False))))


def test_case_ids_are_unique():
    assert len({t[0] for t in TABLE}) == len(TABLE)


@pytest.mark.parametrize("case", TABLE, ids=[t[0] for t in TABLE])
def test_plan_against_the_stub_model(plans, case):
    """the plan, or the status and text — and the stub's row pointer is null again after the call, accepted or refused"""
    tag, _, _, want = case
    assert plans[tag] == want
    assert " rows=null" in plans[tag]


def test_plan_probe_is_clean_under_address_and_ub_sanitizers():
    """the same stand-alone program built with -fsanitize=address,undefined, once over the whole table: same lines, no report"""
    lines = _run(_build(sanitize=True))
    assert lines == [t[3] for t in TABLE]


# ------------------------------------------------------------------ mppi_create before the device check ----------------------
def _cfg(**kw):
    cfg = capi.MppiConfig(model=b"cartpole", controller=VANILLA, num_rollouts=64, num_timesteps=8, dt=0.02, lambda_=1.0, alpha=0.0,
                          num_iters=1, seed=1, noise_source=0, block_x=0, block_y=0, device=0, stream=None, rank=0, world_size=1,
                          save_samples=0, kernel_variant=AUTO, force_exchange=0)
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


SAMPLER_TEXT = ("mppi_create: the Vanilla, Tube and Robust controllers take MPPI_SAMPLER_GAUSSIAN or MPPI_SAMPLER_NLN, "
                "MPPI_CONTROLLER_COLORED takes MPPI_SAMPLER_COLORED only")
SIZES_TEXT = "mppi_create: num_rollouts, num_timesteps, dt, lambda, num_iters must be > 0"
RANK_TEXT = "mppi_create: rank/world_size invalid or num_rollouts not divisible by world_size"

# (id, cfg or None, sampler kind, pass an out pointer, text) — every one is MPPI_ERR_INVALID_ARG
EARLY = [
    ("null-cfg", None, m.MPPI_SAMPLER_GAUSSIAN, True, "mppi_create: null argument"),
    ("null-out", _cfg(), m.MPPI_SAMPLER_GAUSSIAN, False, "mppi_create: null argument"),
    ("null-model", _cfg(model=None), m.MPPI_SAMPLER_GAUSSIAN, True, "mppi_create: null argument"),
    ("colored-sampler-on-vanilla", _cfg(), m.MPPI_SAMPLER_COLORED, True, SAMPLER_TEXT),
    ("gaussian-sampler-on-colored", _cfg(controller=COLORED), m.MPPI_SAMPLER_GAUSSIAN, True, SAMPLER_TEXT),
    ("nln-sampler-on-colored", _cfg(controller=COLORED), m.MPPI_SAMPLER_NLN, True, SAMPLER_TEXT),
    ("unknown-sampler", _cfg(), 9, True, SAMPLER_TEXT),
    ("zero-rollouts", _cfg(num_rollouts=0), m.MPPI_SAMPLER_GAUSSIAN, True, SIZES_TEXT),
    ("negative-timesteps", _cfg(num_timesteps=-1), m.MPPI_SAMPLER_GAUSSIAN, True, SIZES_TEXT),
    ("zero-dt", _cfg(dt=0.0), m.MPPI_SAMPLER_GAUSSIAN, True, SIZES_TEXT),
    ("nan-lambda", _cfg(lambda_=float("nan")), m.MPPI_SAMPLER_GAUSSIAN, True, SIZES_TEXT),
    ("zero-iters", _cfg(num_iters=0), m.MPPI_SAMPLER_GAUSSIAN, True, SIZES_TEXT),
    ("kernel-variant-3", _cfg(kernel_variant=3), m.MPPI_SAMPLER_GAUSSIAN, True, "mppi_create: unknown kernel_variant"),
    ("kernel-variant-negative", _cfg(kernel_variant=-1), m.MPPI_SAMPLER_GAUSSIAN, True, "mppi_create: unknown kernel_variant"),
    ("rank-negative", _cfg(rank=-1), m.MPPI_SAMPLER_GAUSSIAN, True, RANK_TEXT),
    ("rank-beyond-world", _cfg(rank=2, world_size=2), m.MPPI_SAMPLER_GAUSSIAN, True, RANK_TEXT),
    ("rollouts-not-divisible", _cfg(num_rollouts=65, world_size=2), m.MPPI_SAMPLER_GAUSSIAN, True, RANK_TEXT),
    # precedence: the sampler mismatch before the sizes, the sizes before the variant, the variant before the rank
    ("sampler-before-sizes", _cfg(num_rollouts=0), m.MPPI_SAMPLER_COLORED, True, SAMPLER_TEXT),
    ("sizes-before-variant", _cfg(num_iters=0, kernel_variant=3), m.MPPI_SAMPLER_GAUSSIAN, True, SIZES_TEXT),
    ("variant-before-rank", _cfg(kernel_variant=3, rank=-1), m.MPPI_SAMPLER_GAUSSIAN, True, "mppi_create: unknown kernel_variant"),
]


@pytest.mark.parametrize("case", EARLY, ids=[e[0] for e in EARLY])
def test_create_argument_checks_come_before_the_device(lib, case):
    """null arguments, sampler / controller mismatch, non-positive sizes, unknown kernel_variant, bad rank or world size:
    refused with MPPI_ERR_INVALID_ARG and the exact text, with or without a device"""
    _, cfg, sampler, with_out, text = case
    out = capi.H(0x1234)
    st = lib.mppi_create_with_sampler(C.byref(cfg) if cfg is not None else None, sampler, C.byref(out) if with_out else None)
    assert st == m.MPPI_ERR_INVALID_ARG
    assert lib.mppi_last_error(None).decode() == text
    if with_out and cfg is not None and cfg.model is not None:
        assert out.value is None  # *out is cleared once the three pointers are known to be there


def test_mppi_create_refuses_a_null_configuration(lib):
    out = capi.H()
    assert lib.mppi_create(None, C.byref(out)) == m.MPPI_ERR_INVALID_ARG
    assert lib.mppi_last_error(None).decode() == "mppi_create: null argument"
