"""tests/native_build.py itself: what "fresh" means, what a failed or timed-out compile leaves behind, and that start() +
finish() is build().  g++ on a three-line source with a one-line header; no GPU, no hipcc."""
import json
import os
import time

import pytest

import native_build as nb


def _stat(path):
    st = os.stat(path)
    return st.st_mtime_ns, st.st_ino


@pytest.fixture
def unit(tmp_path):
    (tmp_path / "answer.h").write_text("#define ANSWER 42\n")
    (tmp_path / "probe.cpp").write_text('#include "answer.h"\n#include <cstdio>\nint main() { return std::printf("%d\\n", ANSWER + EXTRA) < 0; }\n')
    src, hdr = str(tmp_path / "probe.cpp"), str(tmp_path / "answer.h")
    return SimpleUnit(str(tmp_path / "out" / "probe"), [nb.cxx(), "-O0", "-DEXTRA=0", src], [src, hdr], tmp_path)


class SimpleUnit:
    def __init__(self, target, cmd, deps, dir):
        self.target, self.cmd, self.deps, self.dir = target, cmd, deps, dir

    def build(self, cmd=None, **kw):
        return nb.build(self.target, cmd or self.cmd, self.deps, "probe", **kw)

    def files(self):
        return sorted(os.listdir(os.path.dirname(self.target)))


def test_fresh_means_exists_newer_than_deps_and_same_command(unit):
    assert unit.build() == unit.target and os.access(unit.target, os.X_OK)  # the first call builds
    assert json.load(open(unit.target + ".cmd")) == unit.cmd
    assert unit.files() == ["probe", "probe.cmd"]
    before = _stat(unit.target), _stat(unit.target + ".cmd")
    unit.build()  # nothing changed: the compiler does not run
    assert (_stat(unit.target), _stat(unit.target + ".cmd")) == before
    later = time.time() + 5
    os.utime(unit.deps[1], (later, later))  # a newer dependency rebuilds
    unit.build()
    assert _stat(unit.target)[1] != before[0][1]
    os.utime(unit.deps[1], (later - 3600, later - 3600))
    os.utime(unit.deps[0], (later - 3600, later - 3600))
    before = _stat(unit.target)
    unit.build()
    assert _stat(unit.target) == before
    flagged = [a.replace("-DEXTRA=0", "-DEXTRA=1") for a in unit.cmd]  # one flag changed rebuilds, and the sidecar says so
    unit.build(flagged)
    assert _stat(unit.target) != before and json.load(open(unit.target + ".cmd")) == flagged
    assert unit.files() == ["probe", "probe.cmd"]


def test_failed_compile_raises_and_leaves_the_previous_artefact(unit):
    unit.build()
    kept = open(unit.target, "rb").read(), open(unit.target + ".cmd", "rb").read(), _stat(unit.target)
    (unit.dir / "probe.cpp").write_text('#include "answer.h"\nint main() { return no_such_name; }\n')
    with pytest.raises(nb.BuildError) as e:
        unit.build()
    assert "probe" in str(e.value) and "no_such_name" in str(e.value) and "-DEXTRA=0" in str(e.value), str(e.value)
    assert (open(unit.target, "rb").read(), open(unit.target + ".cmd", "rb").read(), _stat(unit.target)) == kept
    assert unit.files() == ["probe", "probe.cmd"]  # no temporary


def test_compile_beyond_its_time_limit_is_killed(unit):
    t0 = time.time()
    job = nb.start(unit.target, ["sh", "-c", "touch $2; sleep 60", "compiler"], unit.deps, "sleeper")  # $1 $2: -o <temporary>
    with pytest.raises(nb.BuildError) as e:
        nb.finish(job, timeout=0.5)
    assert time.time() - t0 < 10 and "sleeper" in str(e.value) and "no end within" in str(e.value)
    assert job.proc.poll() is not None  # killed, the shell's child with it (one process group)
    assert unit.files() == []


def test_start_then_finish_is_build(unit):
    job = nb.start(unit.target, unit.cmd, unit.deps, "probe")
    assert nb.finish(job) == unit.target and json.load(open(unit.target + ".cmd")) == unit.cmd
    split = open(unit.target, "rb").read()
    before = _stat(unit.target)
    assert nb.finish(nb.start(unit.target, unit.cmd, unit.deps, "probe")) == unit.target and _stat(unit.target) == before  # fresh
    os.remove(unit.target)
    unit.build()
    assert open(unit.target, "rb").read() == split and unit.files() == ["probe", "probe.cmd"]


def test_oracle_flags_are_the_makefiles():
    """oracle_flags() reads oracle/Makefile's CXXFLAGS line; the flag every 0-ulp assertion rests on is in it"""
    line = [l for l in open(os.path.join(nb.ORACLE, "Makefile")) if l.startswith("CXXFLAGS")]
    assert len(line) == 1 and nb.oracle_flags() == line[0].split("?=")[1].split()
    assert "-ffp-contract=off" in nb.oracle_flags() and "-std=c++17" in nb.oracle_flags()
    assert nb.oracle_lib("x.cpp")[1:1 + len(nb.oracle_flags())] == nb.oracle_flags()
