"""What mppi_create decides, for every in-tree registration, held to a recording of the commit before the launch plan moved
into mppi-generic_amd/csrc/launch_plan.hpp (tests/golden/create_table.json).

Per (model, sampler, controller): kernel_variant in {AUTO, FUSED, PIPELINE} x block in {unset, the first registered shape for
the controller's bz} x MPPI_AMD_ROWS_IN_HBM in {unset, 1} x the horizons of the fixture — T = 8 and the T on each side of every
point below T_MAX at which the outcome of one of those requests changes (the rows and the output ring overflowing the LDS, the
rows alone, Robust MPPI's 64 -> 32 -> HBM), found by bisection when the fixture was recorded.  K = 64: one block; K = 128 for a
Tube controller on a model with the folded pipeline, whose blocks hold 32 rollouts.  One mppi_compute_control on in-kernel Philox
noise, then mppi_get_launch_info — or, for a refusal, the status and the text.  Three configurations with two faults each pin
which one is reported.

    python tests/test_create_table.py --record [path]     writes the fixture from the library in the tree it is run in

The fixture is recorded on the parent of a change to mppi_create, never on the change itself, and not edited by hand.
"""
import ctypes as C
import json
import os
import sys

import pytest

if __name__ == "__main__":
    _repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_repo, os.path.join(_repo, "oracle"), os.path.join(_repo, "tests")):
        sys.path.insert(0, _p)

import mppi_generic_amd as m
from mppi_generic_amd import capi
from common import SEED, make_engine
from kernel_forms import BUILDERS, env_override, registrations, robust_gains

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "create_table.json")
NLN = m.MPPI_SAMPLER_NLN
SAMPLER_NAMES = {m.MPPI_SAMPLER_GAUSSIAN: "gaussian", m.MPPI_SAMPLER_COLORED: "colored", NLN: "nln"}
KINDS = {"vanilla": 0, "tube": 1, "robust": 2, "colored": 3}  # mppi_controller_kind
VARIANTS = (m.MPPI_KERNEL_AUTO, m.MPPI_KERNEL_FUSED, m.MPPI_KERNEL_PIPELINE)
T_MAX_TC = 1400  # horizons up to T * C = 1400: past the rows of 64 and of 2 x 64 slots (T * C = 640, 320) and of Robust's 2 x 32


# ------------------------------------------------------------------ the table's axes ------------------------------------
def pairs():
    """(key, name, sampler, description, controller) of every in-tree registration with each controller it admits"""
    regs = registrations() + [(n, NLN, m.describe_model(n, NLN)) for n in m.list_models() if m.describe_model(n, NLN) is not None]
    out = []
    for name, sampler, d in regs:
        if name not in BUILDERS:
            continue  # a plugin another test module has loaded: not part of the library
        controllers = ["colored"] if sampler == m.MPPI_SAMPLER_COLORED else ["vanilla", "tube"] + (["robust"] if d["rmppi"] else [])
        for ctl in controllers:
            out.append(("%s|%s|%s" % (name, SAMPLER_NAMES[sampler], ctl), name, sampler, d, ctl))
    return out


def requests(d, ctl):
    """(kernel_variant, block_x, block_y, rows-in-HBM switch) of a pair, in the order of the fixture's rows"""
    bz = 2 if ctl in ("tube", "robust") else 1
    first = next(((s[0], s[1]) for s in d["shapes"] if s[2] == bz), None)
    blocks = [(0, 0)] + ([first] if first else [])
    return [(v, b[0], b[1], hbm) for v in VARIANTS for b in blocks for hbm in (0, 1)]


def rollouts(d, ctl):
    return 128 if ctl == "tube" and d["pipeline_fold"] else 64


# ------------------------------------------------------------------ one row ---------------------------------------------
def _engine(name, sampler, ctl, K, T, kw):
    D = 2 if ctl in ("tube", "robust") else 1
    cfg = BUILDERS[name](K, T, D)
    cfg["D"] = D
    cfg["num_iters"] = 1
    kw = dict(kw, sampler=sampler)
    if ctl == "colored":
        cfg["colored"] = ([1.0, 0.5][:len(cfg["control_cost_coeff"])], 0.97, 0.0)
    if ctl != "robust":
        return cfg, make_engine(cfg, tube=D == 2, **kw)
    eng = m.RobustMPPIController(cfg["model"], K, T, cfg["dt"], cfg["lambda_"], cfg["alpha"], 1, seed=SEED, **kw)
    if cfg["dyn"] is not None:
        eng.setDynamicsParams(cfg["dyn"])
    eng.setCostParams(cfg["cost"])
    for blob, arr in cfg.get("blobs", {}).items():
        eng.setModelBlob(blob, arr)
    if cfg["ranges"] is not None:
        eng.setControlRanges(cfg["ranges"])
    eng.setSamplingParams(cfg["std_dev"], [0.2, 0.1][:len(cfg["control_cost_coeff"])], cfg.get("pure_pct", 0.01), cfg.get("decay", 1.0))
    eng.setRMPPIParams(1000.0, 3, K // 3)
    return cfg, eng


def outcome(name, sampler, ctl, K, T, request):
    """what the request gets: the launch info of one computeControl, or the status and text of the refusal"""
    variant, bx, by, hbm = request
    try:
        with env_override(MPPI_AMD_ROWS_IN_HBM="1" if hbm else None):
            cfg, eng = _engine(name, sampler, ctl, K, T, dict(kernel_variant=variant, block_x=bx, block_y=by))
    except m.MPPIError as e:
        return {"status": e.status, "error": str(e)}
    try:
        eng.setSeed(7)
        if ctl == "robust":
            eng.updateImportanceSamplingControl(cfg["x0"], 1)
            eng.setFeedbackGains(robust_gains(T, eng.STATE_DIM, eng.CONTROL_DIM))
        eng.computeControl(cfg["x0"], 1)
        info = eng.getLaunchInfo()
        return {"family": info["family"], "block": list(info["block"]), "rows_in_hbm": info["rows_in_hbm"],
                "streamed_merge": info["streamed_merge"]}
    except m.MPPIError as e:
        return {"created": True, "status": e.status, "error": str(e)}
    finally:
        eng.close()


def raw_create(model, controller, sampler, K, T, variant=0, bx=0, by=0, noise_source=0, hbm=0):
    """mppi_create_with_sampler alone -> (status, text of mppi_last_error(NULL) for a refusal); the handle goes at once"""
    lib = m.load_library()
    cfg = capi.MppiConfig(model.encode(), controller, K, T, 0.02, 1.0, 0.0, 1, 1, noise_source, bx, by, 0, None, 0, 1, 0, variant, 0)
    h = capi.H()
    with env_override(MPPI_AMD_ROWS_IN_HBM="1" if hbm else None):
        st = lib.mppi_create_with_sampler(C.byref(cfg), sampler, C.byref(h))
    if st == 0:
        lib.mppi_destroy(h)
        return {"status": 0}
    return {"status": st, "error": lib.mppi_last_error(None).decode()}


# ------------------------------------------------------------------ the test --------------------------------------------
def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


TABLE = _fixture() if os.path.exists(FIXTURE) else {"pairs": {}, "double_faults": []}


def test_fixture_covers_every_in_tree_registration_and_controller(gpu):
    assert sorted(TABLE["pairs"]) == sorted(p[0] for p in pairs())
    assert len(TABLE["double_faults"]) == 3


@pytest.mark.parametrize("key", sorted(TABLE["pairs"]))
def test_create_gives_what_the_parent_commit_gave(gpu, key):
    """every (kernel_variant, block, MPPI_AMD_ROWS_IN_HBM, T) of the pair: the same launch, or the same status and text"""
    entry = TABLE["pairs"][key]
    name, sampler_name, ctl = key.split("|")
    sampler = {v: k for k, v in SAMPLER_NAMES.items()}[sampler_name]
    d = m.describe_model(name, sampler)
    assert d is not None, key
    reqs = requests(d, ctl)
    assert [list(r) for r in reqs] == entry["requests"], "the registered shapes changed: record the fixture again on the parent"
    K = entry["K"]
    assert K == rollouts(d, ctl)
    wrong = []
    for T, row in zip(entry["horizons"], entry["rows"]):
        assert len(row) == len(reqs)
        for request, want in zip(reqs, row):
            got = outcome(name, sampler, ctl, K, T, request)
            if got != want:
                wrong.append((T, request, got, want))
    assert not wrong, "%d of %d differ, the first: T=%d request=%s\n got  %s\n want %s" % (
        (len(wrong), len(reqs) * len(entry["horizons"])) + wrong[0])


@pytest.mark.parametrize("case", TABLE["double_faults"], ids=[c["id"] for c in TABLE["double_faults"]])
def test_which_of_two_faults_is_reported(gpu, case):
    assert raw_create(**case["create"]) == case["outcome"]


# ------------------------------------------------------------------ recording -------------------------------------------
def _signature(o):
    """what has to change for a horizon to count as a boundary: the launch, or the status (a refusal's text carries byte counts)"""
    return json.dumps(o if "family" in o else {"status": o["status"], "created": o.get("created", False)}, sort_keys=True)


def _boundaries(sig, lo, hi):
    """the T in [lo, hi) with sig(T) != sig(T + 1), by bisection (the outcome changes with T through LDS sizes that grow with it)"""
    if sig(lo) == sig(hi):
        return []
    if hi == lo + 1:
        return [lo]
    mid = (lo + hi) // 2
    return _boundaries(sig, lo, mid) + _boundaries(sig, mid, hi)


def record(path):
    lib = m.load_library()
    assert lib.mppi_device_count() > 0, "recording needs a device"
    table = {"recorded_from": lib.mppi_source_hash().decode(), "pairs": {}, "double_faults": []}
    overflow = None
    for key, name, sampler, d, ctl in pairs():
        K, reqs = rollouts(d, ctl), requests(d, ctl)
        channels = len(BUILDERS[name](K, 8, 1)["control_cost_coeff"])
        t_max = -(-T_MAX_TC // channels)
        seen = {}

        def at(T, request):
            if (T, request) not in seen:
                seen[(T, request)] = outcome(name, sampler, ctl, K, T, request)
            return seen[(T, request)]
        horizons = {8}
        for request in reqs:
            for b in _boundaries(lambda T: _signature(at(T, request)), 8, t_max):
                horizons.update((b, b + 1))
        horizons = sorted(horizons)
        rows = [[at(T, request) for request in reqs] for T in horizons]
        table["pairs"][key] = {"K": K, "requests": [list(r) for r in reqs], "horizons": horizons, "rows": rows}
        for T, row in zip(horizons, rows):
            for request, o in zip(reqs, row):
                if overflow is None and o.get("status") == m.MPPI_ERR_LDS_OVERFLOW and not o.get("created"):
                    overflow = dict(model=name, controller=KINDS[ctl], sampler=sampler, K=K, T=T, variant=request[0], bx=request[1],
                                    by=request[2], hbm=request[3])
        print("%-60s K=%d horizons %s (%d probes)" % (key, K, horizons, len(seen)), flush=True)
    if overflow is None:  # no request of the table overflows at mppi_create: look further out, creation only
        for T in (5000, 50000, 200000):
            for model, ctl, sampler, variant, bx in (("double_integrator_robust", "robust", 0, 1, 64), ("double_integrator_robust", "robust", 0, 2, 0),
                                                     ("cartpole", "colored", 1, 2, 64), ("cartpole", "colored", 1, 1, 64),
                                                     ("cartpole", "vanilla", 0, 2, 64), ("autorally_nn", "vanilla", 0, 2, 64)):
                args = dict(model=model, controller=KINDS[ctl], sampler=sampler, K=64, T=T, variant=variant, bx=bx, by=0, hbm=0)
                if overflow is None and raw_create(**args).get("status") == m.MPPI_ERR_LDS_OVERFLOW:
                    overflow = args
    faults = [("unknown-controller-and-unregistered-model", dict(model="no_such_model", controller=9, sampler=0, K=64, T=8)),
              ("pipeline-on-robust-and-block_x-16", dict(model="double_integrator_robust", controller=KINDS["robust"], sampler=0, K=64, T=8,
                                                         variant=m.MPPI_KERNEL_PIPELINE, bx=16))]
    if overflow is not None:
        faults.insert(0, ("unknown-noise_source-and-lds-overflow", dict(overflow, noise_source=7)))
    else:
        print("no configuration overflows the LDS at mppi_create: the first double fault is not recorded", flush=True)
    for tag, args in faults:
        table["double_faults"].append({"id": tag, "create": args, "outcome": raw_create(**args)})
        print(tag, table["double_faults"][-1]["outcome"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(table, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote %s: %d pairs, %d rows" % (path, len(table["pairs"]), sum(len(e["rows"]) * len(e["requests"]) for e in table["pairs"].values())))


if __name__ == "__main__":
    if "--record" in sys.argv:
        i = sys.argv.index("--record")
        record(sys.argv[i + 1] if len(sys.argv) > i + 1 else FIXTURE)
    else:
        sys.exit("usage: python tests/test_create_table.py --record [path]")
