"""mppi_evaluate_controls / mppi_warm_start, the parts that need no device: the argument checks and the warm-start choice of
include/mppi_amd/engine/evaluate_host.hpp in a stand-alone program (tests/probes/evaluate_host_probe.cpp; once more under the
address and undefined-behaviour sanitizers), the choice against a pure-Python reference, the exported and bound symbols, and the
refusals the library decides before any HIP call.  A Robust handle's MPPI_ERR_UNSUPPORTED needs a handle, hence a device: its text
is checked here, its status in tests/test_evaluate_gpu.py."""
import subprocess

import numpy as np
import pytest

import mppi_generic_amd as m
import native_build as nb
from evaluate_cases import choice_reference

INF, NAN = np.float32(np.inf), np.float32(np.nan)
N_MAX = 65536

ROBUST_TEXT = ("mppi_warm_start: the nominal system of a Robust MPPI handle is chosen by its candidate-state search; installing a "
               "control sequence under it is not supported")
HYST_TEXT = "mppi_warm_start: the hysteresis has to be finite and >= 0"


def count_text(x0_count, n):
    return ("mppi_evaluate_controls: x0_count = %d is neither 1 (one initial state for every row) nor n = %d (one per row)"
            % (x0_count, n))


# (x0 there, x0_count, u there, n, expected): every refusal of checkEvaluateArgs with its text, and the accepted edges
ARGS = [
    (1, 1, 1, 1, "ok"),
    (1, 1, 1, N_MAX, "ok"),
    (1, N_MAX, 1, N_MAX, "ok"),
    (1, 7, 1, 7, "ok"),
    (1, 1, 1, 0, "mppi_evaluate_controls: n = 0 is outside [1, 65536]"),
    (1, 1, 1, -3, "mppi_evaluate_controls: n = -3 is outside [1, 65536]"),
    (1, 1, 1, N_MAX + 1, "mppi_evaluate_controls: n = 65537 is outside [1, 65536]"),
    (0, 1, 1, 4, "mppi_evaluate_controls: null x0"),
    (1, 1, 0, 4, "mppi_evaluate_controls: null u"),
    (1, 0, 1, 4, count_text(0, 4)),
    (1, 2, 1, 4, count_text(2, 4)),
    (1, 5, 1, 4, count_text(5, 4)),
    (1, -1, 1, 4, count_text(-1, 4)),
    # precedence: n, then the pointers, then the count
    (0, 9, 0, 0, "mppi_evaluate_controls: n = 0 is outside [1, 65536]"),
    (0, 9, 0, 4, "mppi_evaluate_controls: null x0"),
    (1, 9, 0, 4, "mppi_evaluate_controls: null u"),
]

# (x0 there, candidates there, n, hysteresis, expected)
WARM = [
    (1, 1, 1, 0.0, "ok"),
    (1, 1, N_MAX - 1, 2.5, "ok"),
    (1, 1, 0, 0.0, "mppi_warm_start: n = 0 is outside [1, 65535]"),
    (1, 1, N_MAX, 0.0, "mppi_warm_start: n = 65536 is outside [1, 65535]"),
    (0, 1, 3, 0.0, "mppi_warm_start: null x0"),
    (1, 0, 3, 0.0, "mppi_warm_start: null candidates"),
    (1, 1, 3, -1e-30, HYST_TEXT),
    (1, 1, 3, -INF, HYST_TEXT),
    (1, 1, 3, INF, HYST_TEXT),
    (1, 1, 3, NAN, HYST_TEXT),
    (1, 1, 3, -0.0, "ok"),
]

# (id, hysteresis, costs[0] = the current sequence's, then the candidates', expected by hand)
CHOICE = [
    ("cheapest-candidate-wins", 0.0, [5, 7, 3, 4], 1),
    ("ties-among-candidates-to-the-lower-index", 0.0, [5, 3, 3, 3], 0),
    ("tie-with-the-current-sequence-keeps-it", 0.0, [3, 3, 3], -1),
    ("exactly-hysteresis-cheaper-is-not-installed", 2.0, [5, 3, 4], -1),
    ("one-ulp-more-than-hysteresis-cheaper-is", 2.0, [5, np.nextafter(np.float32(3), np.float32(0)), 4], 0),
    ("within-the-hysteresis", 2.0, [5, 4, 3.5], -1),
    ("beyond-the-hysteresis", 2.0, [5, 4, 2.5], 1),
    ("nan-current-any-number-wins", 100.0, [NAN, 9, 8, NAN], 1),
    ("nan-current-inf-candidate-wins", 0.0, [NAN, NAN, INF], 1),
    ("nan-current-all-nan-candidates", 0.0, [NAN, NAN, NAN], -1),
    ("all-nan-candidates", 0.0, [5, NAN, NAN], -1),
    ("nan-candidates-are-last", 0.0, [5, NAN, 4, NAN, 4], 1),
    ("inf-current-finite-candidate", 3.0, [INF, 1e30, 7], 1),
    ("inf-current-inf-candidates", 0.0, [INF, INF, INF], -1),
    ("inf-candidates-lose", 0.0, [5, INF, INF], -1),
    ("minus-inf-candidate", 1.0, [5, 2, -INF], 1),
    ("minus-inf-current", 0.0, [-INF, -INF, 0], -1),
    ("negative-zero-ties-with-zero", 0.0, [0.0, -0.0], -1),
    ("single-candidate", 0.5, [1.0, 0.25], 0),
    ("hysteresis-lost-to-rounding", 1e-9, [5, 5], -1),
]


def bits(x):
    return "%08x" % int(np.array(x, np.float32).view(np.uint32))


def _lines():
    text = ["args %d %d %d %d" % c[:4] for c in ARGS]
    text += ["warm %d %d %d %s" % (c[0], c[1], c[2], bits(c[3])) for c in WARM]
    text += ["choice %s %d %s" % (bits(h), len(c) - 1, " ".join(bits(v) for v in c)) for _, h, c, _ in CHOICE]
    text += ["robust"]
    return text


def _run(exe):
    r = subprocess.run([exe], input="\n".join(_lines()) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    out = r.stdout.splitlines()
    assert len(out) == len(ARGS) + len(WARM) + len(CHOICE) + 1, r.stdout
    return out


@pytest.fixture(scope="module")
def answers():
    return _run(nb.build_plan_probe("evaluate_host_probe", sanitize=False))


@pytest.mark.parametrize("i", range(len(ARGS)))
def test_check_evaluate_args(answers, i):
    assert answers[i] == ARGS[i][4]


@pytest.mark.parametrize("i", range(len(WARM)))
def test_check_warm_start_args(answers, i):
    assert answers[len(ARGS) + i] == WARM[i][4]


@pytest.mark.parametrize("case", CHOICE, ids=[c[0] for c in CHOICE])
def test_warm_start_choice(answers, case):
    """the header's rule, the pure-Python reference and the value worked out by hand agree"""
    tag, hyst, costs, want = case
    got = int(answers[len(ARGS) + len(WARM) + [c[0] for c in CHOICE].index(tag)])
    assert choice_reference(costs, hyst) == want
    assert got == want


def test_warm_start_choice_on_random_costs_with_ties_and_specials():
    """4000 drawn cases from a small alphabet of costs (many ties, NaN, both infinities) against the reference"""
    rng = np.random.default_rng(11)
    alphabet = np.array([-INF, -1.0, 0.0, 1.0, 1.5, 2.0, 3.0, INF, NAN], np.float32)
    cases = []
    for _ in range(4000):
        n = int(rng.integers(1, 6))
        cases.append((np.float32(rng.choice([0.0, 0.5, 1.0, 2.0])), alphabet[rng.integers(0, alphabet.size, n + 1)]))
    text = "".join("choice %s %d %s\n" % (bits(h), c.size - 1, " ".join(bits(v) for v in c)) for h, c in cases)
    r = subprocess.run([nb.build_plan_probe("evaluate_host_probe", sanitize=False)], input=text, capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stderr[-3000:]
    got = [int(v) for v in r.stdout.split()]
    want = [choice_reference(c, h) for h, c in cases]
    assert got == want
    assert {-1, 0, 1, 2, 3}.issubset(set(want))


def test_robust_refusal_text(answers):
    assert answers[-1] == ROBUST_TEXT


def test_host_checks_under_the_sanitizers():
    """the same stand-alone program built with -fsanitize=address,undefined, once over every case: same lines, no report"""
    plain = _run(nb.build_plan_probe("evaluate_host_probe", sanitize=False))
    assert _run(nb.build_plan_probe("evaluate_host_probe", sanitize=True)) == plain


# ------------------------------------------------------------------ through the library, before any HIP call -----------------
def test_declared_symbols_are_exported_and_bound(lib):
    for name in ("mppi_evaluate_controls", "mppi_warm_start"):
        assert hasattr(lib, name), "libmppi_amd.so does not export " + name
        assert name in m.SIGNATURES


def _buf(n=4):
    return np.zeros(n, np.float32)


@pytest.mark.parametrize("i", [i for i, c in enumerate(ARGS) if c[4] != "ok"])
def test_evaluate_refusals_need_no_handle_and_no_device(lib, i):
    """the arguments are checked before the handle: the refusal reads the same with or without one (mppi_last_error(NULL))"""
    x0, x0_count, u, n, text = ARGS[i]
    a, b = _buf(), _buf()
    st = lib.mppi_evaluate_controls(None, a.ctypes.data if x0 else None, x0_count, b.ctypes.data if u else None, n, None, None)
    assert st == m.MPPI_ERR_INVALID_ARG
    assert lib.mppi_last_error(None).decode() == text


@pytest.mark.parametrize("i", [i for i, c in enumerate(WARM) if c[4] != "ok"])
def test_warm_start_refusals_need_no_handle_and_no_device(lib, i):
    x0, cand, n, hyst, text = WARM[i]
    a, b = _buf(), _buf()
    st = lib.mppi_warm_start(None, a.ctypes.data if x0 else None, b.ctypes.data if cand else None, n, float(hyst), None, None)
    assert st == m.MPPI_ERR_INVALID_ARG
    assert lib.mppi_last_error(None).decode() == text


def test_a_null_handle_is_refused_with_its_own_text(lib):
    a, b = _buf(), _buf()
    assert lib.mppi_evaluate_controls(None, a.ctypes.data, 1, b.ctypes.data, 1, None, None) == m.MPPI_ERR_INVALID_ARG
    assert lib.mppi_last_error(None).decode() == "mppi_evaluate_controls: null handle"
    assert lib.mppi_warm_start(None, a.ctypes.data, b.ctypes.data, 1, 0.0, None, None) == m.MPPI_ERR_INVALID_ARG
    assert lib.mppi_last_error(None).decode() == "mppi_warm_start: null handle"
