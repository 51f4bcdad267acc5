"""The CPU restatement of the quadrotor model (quadrotor_oracle.cpp) for the tests: build helper and ctypes loader.

quadrotor_oracle.cpp is compiled together with the unchanged oracle/oracle_capi.cpp into ONE library
(tests/quadrotor_oracle/_build/libquadrotor_oracle.so, with the flags of oracle/Makefile), so the handle its factory returns is
an oracle::Controller of that library and every oracle_* entry point takes it.  QuadrotorOracle is pyoracle.Oracle on that
handle: the methods the tests use are declared here for this library.
"""
import ctypes as C
import os
import subprocess

import numpy as np

import pyoracle as po

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
ORACLE = os.path.join(REPO, "oracle")
LIB = os.path.join(HERE, "_build", "libquadrotor_oracle.so")
# oracle/Makefile's CXXFLAGS: -ffp-contract=off keeps det::fma() the only fused operation
CXXFLAGS = ["-O2", "-std=c++17", "-fPIC", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-Wall",
            "-Wno-unused-parameter"]
_f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
_lib = None


def build(force=False):
    srcs = [os.path.join(HERE, "quadrotor_oracle.cpp"), os.path.abspath(__file__)]
    srcs += [os.path.join(ORACLE, f) for f in os.listdir(ORACLE) if f.endswith((".cpp", ".hpp"))]
    srcs += [os.path.join(REPO, "include", "mppi_amd", f) for f in ("det_math.h", "model_params.h")]
    if force or not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in srcs):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        cmd = [os.environ.get("CXX", "g++")] + CXXFLAGS + ["-I" + os.path.join(REPO, "include"), "-I" + ORACLE, "-shared",
               os.path.join(ORACLE, "oracle_capi.cpp"), os.path.join(HERE, "quadrotor_oracle.cpp"), "-o", LIB + ".tmp"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("quadrotor oracle build failed:\n" + r.stdout + r.stderr)
        os.replace(LIB + ".tmp", LIB)
    return LIB


PLUGIN_MATH = os.path.join(HERE, "_build", "libplugin_math_host.so")
_plugin_math = None


def plugin_math():
    """the product's own helpers (plugin/math_utils.hpp) and parameter classes, host side: plugin_math_host.hip through hipcc,
    host code only (no device pass, nothing of the GPU is touched when it is loaded)"""
    global _plugin_math
    if _plugin_math is None:
        src = os.path.join(HERE, "plugin_math_host.hip")
        deps = [src] + [os.path.join(d, f) for d, _, fs in os.walk(os.path.join(REPO, "include")) for f in fs]
        if not os.path.exists(PLUGIN_MATH) or any(os.path.getmtime(s) > os.path.getmtime(PLUGIN_MATH) for s in deps):
            os.makedirs(os.path.dirname(PLUGIN_MATH), exist_ok=True)
            cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "--cuda-host-only", "-O2", "-std=c++17",
                   "-ffp-contract=off", "-fPIC", "-shared", "-I" + os.path.join(REPO, "include"), src, "-o", PLUGIN_MATH + ".tmp"]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError("plugin_math_host build failed:\n" + r.stdout + r.stderr)
            os.replace(PLUGIN_MATH + ".tmp", PLUGIN_MATH)
        L = C.CDLL(PLUGIN_MATH)
        L.plugin_quat_eval.argtypes = [C.c_int, _f32p, _f32p]
        L.plugin_gravity.restype = C.c_float
        L.plugin_default_params.argtypes = [C.c_void_p, C.c_void_p]
        L.plugin_nan_to_max_cost.restype = C.c_float
        L.plugin_nan_to_max_cost.argtypes = [C.c_float]
        _plugin_math = L
    return _plugin_math


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        h = C.c_void_p
        L.quadrotor_oracle_create.restype = h
        L.quadrotor_oracle_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int]
        L.quadrotor_terminal_cost.restype = C.c_float
        L.quadrotor_terminal_cost.argtypes = [h, _f32p]
        L.quadrotor_det_atan2.argtypes = [_f32p, _f32p, _f32p, C.c_int]
        L.quadrotor_quat_eval.argtypes = [C.c_int, _f32p, _f32p]
        # the oracle's own entry points the tests reach through pyoracle.Oracle's methods (oracle/pyoracle.py declares the same)
        L.oracle_destroy.argtypes = [h]
        L.oracle_dims.argtypes = [h] + [C.POINTER(C.c_int)] * 3
        L.oracle_set_dynamics_params.argtypes = [h, C.c_void_p, C.c_size_t]
        L.oracle_set_cost_params.argtypes = [h, C.c_void_p, C.c_size_t]
        L.oracle_state_deriv.argtypes = [h, _f32p, _f32p, _f32p]
        L.oracle_update_state.argtypes = [h, _f32p, _f32p, C.c_float, _f32p]
        L.oracle_state_cost.restype = C.c_float
        L.oracle_state_cost.argtypes = [h, _f32p, C.c_int, C.POINTER(C.c_int)]
        L.oracle_set_control_ranges.argtypes = [h, _f32p]
        L.oracle_set_control_deadband.argtypes = [h, _f32p]
        L.oracle_set_sampler.argtypes = [h, _f32p, _f32p, C.c_float, C.c_float, C.c_int]
        L.oracle_set_independent_noise.argtypes = [h, C.c_int]
        L.oracle_set_time_specific_std_dev.argtypes = [h, C.c_void_p]
        L.oracle_set_controller_params.argtypes = [h, C.c_float, C.c_void_p]
        L.oracle_set_gaussian_controls.argtypes = [h, _f32p, _f32p, C.c_int, C.c_int, _f32p]
        L.oracle_rollout_costs.argtypes = [h, _f32p, _f32p, _f32p, _f32p, C.c_int]
        L.oracle_iterate.argtypes = [h, _f32p, _f32p, _f32p, C.c_int, C.c_int, _f32p]
        L.oracle_state_trajectory.argtypes = [h, _f32p, _f32p, _f32p]
        L.oracle_output_trajectory.argtypes = [h, _f32p, _f32p, _f32p, _f32p]
        L.oracle_model_step.argtypes = [h, _f32p, _f32p, C.c_float]
        L.oracle_model_step_full.argtypes = [h, _f32p, _f32p, C.c_float, _f32p, _f32p, _f32p]
        L.oracle_set_nominal_control.argtypes = [h, _f32p]
        L.oracle_vanilla_compute_control.argtypes = [h, _f32p, C.c_int, _f32p]
        L.oracle_tube_compute_control.argtypes = [h, _f32p, C.c_int, _f32p]
        L.oracle_vanilla_slide.argtypes = [h, C.c_int]
        L.oracle_tube_slide.argtypes = [h, C.c_int]
        for n in ("control", "nominal_control", "state_traj", "nominal_state_traj", "costs", "weights", "samples", "stats"):
            getattr(L, "oracle_get_" + n).argtypes = [h, _f32p]
        _lib = L
    return _lib


class QuadrotorOracle(po.Oracle):
    """pyoracle.Oracle on the quadrotor restatement (constructor arguments without the model name)"""

    def __init__(self, K, T, D=1, dt=0.01, lambda_=1.0, alpha=0.0, num_iters=1):
        self.L = lib()
        self.h = self.L.quadrotor_oracle_create(K, T, D, dt, lambda_, alpha, num_iters)
        self.S, self.C, self.O = 13, 4, 13
        self.K, self.T, self.D = K, T, D
        self.dt, self.lambda_, self.alpha, self.num_iters = dt, lambda_, alpha, num_iters

    def terminal_cost(self, y):
        return float(self.L.quadrotor_terminal_cost(self.h, np.ascontiguousarray(y, np.float32).reshape(-1)))


def det_atan2(y, x):
    """det::atan2 of the host build, elementwise"""
    y, x = np.broadcast_arrays(np.asarray(y, np.float32), np.asarray(x, np.float32))
    y, x = np.ascontiguousarray(y).reshape(-1), np.ascontiguousarray(x).reshape(-1)
    out = np.empty_like(y)
    lib().quadrotor_det_atan2(y, x, out, y.size)
    return out


class Helpers:
    """the seven helpers on numpy arrays, from one of the two libraries: Helpers(plugin_math().plugin_quat_eval) is the product's
    math_utils.hpp, Helpers(lib().quadrotor_quat_eval) the CPU restatement's own copies"""

    def __init__(self, fn):
        self.fn = fn

    def _call(self, which, args, n_out):
        out = np.zeros(9, np.float32)
        n = self.fn(which, np.ascontiguousarray(np.concatenate([np.ravel(a) for a in args]), np.float32), out)
        assert n == n_out, (which, n)
        return out[:n]

    def quat_multiply(self, q1, q2, normalize=True):
        return self._call(0 if normalize else 6, (q1, q2), 4)

    def quat_inv(self, q):
        return self._call(1, (q,), 4)

    def quat_subtract(self, q1, q2):
        return self._call(2, (q1, q2), 4)

    def quat_to_euler(self, q):
        return self._call(3, (q,), 3)

    def quat_to_dcm(self, q):
        return self._call(4, (q,), 9).reshape(3, 3)

    def omega_to_edot(self, p, q, r, e):
        return self._call(5, ([p, q, r], e), 4)


def plugin_helpers():
    return Helpers(plugin_math().plugin_quat_eval)


def restatement_helpers():
    return Helpers(lib().quadrotor_quat_eval)


MODEL_SRC = os.path.join(REPO, "examples", "quadrotor_model", "quadrotor_model.hip")
MODEL_LIB = os.path.join(REPO, "examples", "_build", "libquadrotor_model.so")


def load_model(m):
    """builds examples/quadrotor_model/quadrotor_model.hip on its own (as tests/test_plugin_model.py builds the pendulum) and
    loads it into the engine's registry with mppi_load_plugin; m is the mppi_generic_amd package"""
    lib_ = m.load_library()
    if "quadrotor" in m.list_models():
        return lib_
    deps = [MODEL_SRC] + [os.path.join(d, f) for d, _, fs in os.walk(os.path.join(REPO, "include")) for f in fs]
    if not os.path.exists(MODEL_LIB) or any(os.path.getmtime(s) > os.path.getmtime(MODEL_LIB) for s in deps):
        os.makedirs(os.path.dirname(MODEL_LIB), exist_ok=True)
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
               "-I" + os.path.join(REPO, "include"), MODEL_SRC, "-o", MODEL_LIB + ".tmp"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        os.replace(MODEL_LIB + ".tmp", MODEL_LIB)
    assert lib_.mppi_load_plugin(MODEL_LIB.encode()) == m.MPPI_OK, lib_.mppi_last_error(None)
    return lib_
