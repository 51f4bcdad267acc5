"""bench.py's plain run: exactly --steps timed iterations, the headline line only, and --dump-outputs reproducible from run
to run (the form in which two builds are compared output for output)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    return subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + list(args), capture_output=True, text=True,
                          timeout=300, cwd=REPO)


def test_dump_outputs_refuses_min_time(tmp_path):
    """repetitions under --min-time depend on measured time, so the dumped iteration would not be reproducible"""
    r = _bench("--dump-outputs", str(tmp_path / "d"), "--min-time", "0.1")
    assert r.returncode == 2 and "--dump-outputs" in r.stderr, r.stderr[-2000:]
    assert not (tmp_path / "d").exists()


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_reproducible_outputs(gpu, tmp_path):
    lines, dumps = [], []
    for run in ("a", "b"):
        d = tmp_path / run
        r = _bench("--gpus", "1", "--steps", "5", "--warmup", "2", "--dump-outputs", str(d))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        out = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(out) == 1, r.stdout[-2000:]
        lines.append(json.loads(out[0]))
        dumps.append({n: np.load(d / (n + ".npy")) for n in ("optimal_control", "trajectory_costs", "statistics")})
    for o in lines:
        assert o["steps"] == 5 and o["warmup"] == 2 and o["timed_region"]["repetitions"] == 1
        assert o["ms_per_step"] > 0 and o["value"] > 0 and o["finite"]
        assert o["unit"] == "MPPI iters/s" and o["higher_is_better"] is True and o["dtype"] == "f32" and o["metric"]
        for key in ("roofline", "cpu_baseline", "compute_control", "autorally_nn"):  # --full only
            assert key not in o, key
    shapes = {"optimal_control": (1, 100, 1), "trajectory_costs": (1, 16384), "statistics": (1, 5)}
    for name, shape in shapes.items():
        a, b = dumps[0][name], dumps[1][name]
        assert a.dtype == np.float32 and a.shape == shape, (name, a.dtype, a.shape)
        assert np.isfinite(a).all() and np.array_equal(a, b), name
