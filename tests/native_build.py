"""The one place under tests/ that runs a compiler: every probe program, host-only library, plugin library, oracle-flavoured
library and C-ABI client a test needs is built by build() (or its split form start() / finish()) from an argument list
spelled once below.

An artefact is fresh iff it exists, is no older than its newest dependency, and its sidecar `<target>.cmd` holds exactly the
argument list about to be run (so a flag, the compiler, HIPCC or CXX changing rebuilds it).  A stale one is compiled into a
name unique to this process and renamed over the target on success; a failed, timed-out or interrupted compile leaves the
previous target and sidecar as they were and nothing else behind."""
import json
import os
import re
import signal
import subprocess
import tempfile
from types import SimpleNamespace

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(REPO, "include")
EXAMPLES = os.path.join(REPO, "examples")
ORACLE = os.path.join(REPO, "oracle")
PROBES = os.path.join(REPO, "tests", "probes")
CSRC = os.path.join(REPO, "mppi-generic_amd", "csrc")
OUT = os.path.join(EXAMPLES, "_build")
ARCH = "--offload-arch=gfx950"
TAIL = 8000  # characters of stdout and of stderr a failure reports


class BuildError(RuntimeError):
    pass


def hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def cxx():
    return os.environ.get("CXX", "g++")


# ------------------------------------------------------------------ dependency sets ------------------------------------
def include_files():
    return [os.path.join(d, f) for d, _, fs in os.walk(INCLUDE) for f in fs]


def library_deps(m):
    """what a program that includes project headers and links libmppi_amd.so depends on, besides its own sources"""
    return [m.library_path()] + include_files()


def oracle_files():
    """what a library that embeds oracle/oracle_capi.cpp depends on, besides its own sources"""
    return ([os.path.join(ORACLE, f) for f in os.listdir(ORACLE) if f.endswith((".cpp", ".hpp"))] +
            [os.path.join(INCLUDE, "mppi_amd", f) for f in ("det_math.h", "model_params.h")])


# ------------------------------------------------------------------ argument lists, each spelled once ------------------
def _link(m):
    lib_dir = os.path.dirname(m.library_path())
    return ["-L" + lib_dir, "-lmppi_amd", "-Wl,-rpath," + lib_dir]


def hip_exe(m, src, *extra):
    """device + host executable against libmppi_amd.so"""
    return [hipcc(), ARCH, "-O3", "-std=c++17", "-ffp-contract=off", "-Werror", "-I" + INCLUDE, *extra, src] + _link(m)


def hip_host(src, *extra):
    """host pass only: no device code, nothing of the GPU is touched by what comes out"""
    return [hipcc(), ARCH, "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-I" + INCLUDE, src]


def hip_host_lib(src, *extra):
    return hip_host(src, "-fPIC", "-shared", *extra)


def hip_plugin(src):
    """a model library for mppi_load_plugin"""
    return [hipcc(), ARCH, "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I" + INCLUDE, src]


def oracle_flags():
    """oracle/Makefile's CXXFLAGS, read from it: -ffp-contract=off keeps det::fma() the only fused operation"""
    return re.search(r"^CXXFLAGS\s*\?=(.*)$", open(os.path.join(ORACLE, "Makefile")).read(), flags=re.M).group(1).split()


def oracle_lib(*srcs):
    """the given sources and the unchanged oracle/oracle_capi.cpp in ONE library, as oracle/Makefile builds the oracle's own"""
    return [cxx()] + oracle_flags() + ["-I" + INCLUDE, "-I" + ORACLE, "-shared", os.path.join(ORACLE, "oracle_capi.cpp"), *srcs]


def abi_client(m, src, opt="-O2"):
    """g++ only (no hipcc, no Eigen) over the C ABI"""
    return [cxx(), "-std=c++11", opt, "-Wall", "-Werror", "-pthread", "-I" + INCLUDE, src] + _link(m)


def hip_syntax_only(src, *extra, timeout=600):
    """the "must compile" / "must be refused" checks: both compiler passes, no code generation, no artefact"""
    return subprocess.run([hipcc(), ARCH, "-std=c++17", "-fsyntax-only", "-I" + INCLUDE, *extra, str(src)],
                          capture_output=True, text=True, timeout=timeout)


# ------------------------------------------------------------------ the build itself -----------------------------------
def _fresh(target, cmd, deps):
    try:
        return (os.path.getmtime(target) >= max(os.path.getmtime(p) for p in deps) and
                json.load(open(target + ".cmd")) == cmd)
    except (OSError, ValueError):
        return False


def _discard(job):
    if job.proc.poll() is None:
        os.killpg(job.proc.pid, signal.SIGKILL)  # hipcc's own children too
        job.proc.wait()
    if os.path.exists(job.tmp):
        os.remove(job.tmp)


def start(target, cmd, deps, what):
    """starts the compile of a stale target without waiting for it; finish() takes what this returns"""
    target, cmd = str(target), [str(a) for a in cmd]
    job = SimpleNamespace(target=target, cmd=cmd, what=what, proc=None)
    if not _fresh(target, cmd, [str(p) for p in deps]):
        os.makedirs(os.path.dirname(target), exist_ok=True)
        job.tmp = "%s.tmp.%d" % (target, os.getpid())
        job.out, job.err = tempfile.TemporaryFile("w+"), tempfile.TemporaryFile("w+")
        job.proc = subprocess.Popen(cmd + ["-o", job.tmp], stdout=job.out, stderr=job.err, start_new_session=True)
    return job


def finish(job, timeout=1800):
    if job.proc is None:
        return job.target
    try:
        rc = job.proc.wait(timeout=timeout)
    except BaseException as e:  # the time limit, Ctrl-C: the compiler does not outlive it
        _discard(job)
        if not isinstance(e, subprocess.TimeoutExpired):
            raise
        rc = "no end within %d s" % timeout
    if rc != 0:
        _discard(job)
        job.out.seek(0), job.err.seek(0)
        raise BuildError("%s build failed (%s):\n%s\n%s%s" % (job.what, rc, " ".join(job.cmd + ["-o", job.tmp]),
                                                             job.out.read()[-TAIL:], job.err.read()[-TAIL:]))
    os.replace(job.tmp, job.target)
    with open(job.target + ".cmd", "w") as f:
        json.dump(job.cmd, f)
    return job.target


def build(target, cmd, deps, what, timeout=1800):
    return finish(start(target, cmd, deps, what), timeout)


# ------------------------------------------------------------------ what several test modules build alike --------------
def example_job(m, name, *extra, deps=()):
    """start()'s arguments for examples/<name>.hip as a program in examples/_build"""
    src = os.path.join(EXAMPLES, name + ".hip")
    return os.path.join(OUT, name), hip_exe(m, src, *extra), [src, *deps] + library_deps(m), name


def build_example(m, name, *extra, deps=(), timeout=1800):
    m.load_library()
    return build(*example_job(m, name, *extra, deps=deps), timeout=timeout)


def build_probe_program(m, name, opt="-O2"):
    """tests/probes/<name>: a .hip with hipcc, its kernels instantiated in the program's own translation unit, a .cpp with
    g++ over the C ABI"""
    m.load_library()
    src = os.path.join(PROBES, name)
    cmd = hip_exe(m, src) if name.endswith(".hip") else abi_client(m, src, opt)
    return build(os.path.join(OUT, os.path.splitext(name)[0]), cmd, [src] + library_deps(m), name)


def build_plan_probe(name, sanitize):
    """tests/probes/<name>.cpp around mppi-generic_amd/csrc/launch_plan.hpp: a stand-alone host program, with the address and
    undefined-behaviour sanitizers if asked (it is run as a child process; nothing is loaded into Python)"""
    src = os.path.join(PROBES, name + ".cpp")
    cmd = [hipcc(), "--cuda-host-only", "-std=c++17", "-Wall", "-Werror", "-I" + INCLUDE, "-I" + CSRC, src]
    cmd += ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    return build(os.path.join(OUT, name + ("_asan" if sanitize else "")), cmd,
                 [src, os.path.join(CSRC, "launch_plan.hpp")] + include_files(), name)


def build_plugin(source, library, deps=()):
    return build(library, hip_plugin(source), [source, *deps] + include_files(), os.path.basename(library))


def load_plugin_model(m, model_name, source, library, deps=()):
    """builds `source` on its own into `library` if stale and loads it into the engine's registry with mppi_load_plugin, unless
    `model_name` is registered already; m is the mppi_generic_amd package"""
    lib = m.load_library()
    if model_name not in m.list_models():
        assert lib.mppi_load_plugin(build_plugin(source, library, deps).encode()) == m.MPPI_OK, lib.mppi_last_error(None)
    return lib
