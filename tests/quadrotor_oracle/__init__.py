"""The CPU restatement of the quadrotor model (quadrotor_oracle.cpp) for the tests: build helper and ctypes loader.

quadrotor_oracle.cpp is compiled together with the unchanged oracle/oracle_capi.cpp into ONE library
(tests/quadrotor_oracle/_build/libquadrotor_oracle.so, by tests/native_build.py with the flags of oracle/Makefile), so the handle its factory returns is
an oracle::Controller of that library and every oracle_* entry point takes it.  QuadrotorOracle is pyoracle.Oracle on that
handle: pyoracle.declare gives this library the oracle's prototypes, the model's own entry points are declared here.
"""
import ctypes as C
import os

import numpy as np

import native_build as nb
import pyoracle as po

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(HERE, "_build", "libquadrotor_oracle.so")
_f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
_lib = None


def build():
    src = os.path.join(HERE, "quadrotor_oracle.cpp")
    return nb.build(LIB, nb.oracle_lib(src), [src, os.path.abspath(__file__)] + nb.oracle_files(), "quadrotor oracle")


PLUGIN_MATH = os.path.join(HERE, "_build", "libplugin_math_host.so")
_plugin_math = None


def plugin_math():
    """the product's own helpers (plugin/math_utils.hpp) and parameter classes, host side: plugin_math_host.hip through hipcc,
    host code only (no device pass, nothing of the GPU is touched when it is loaded)"""
    global _plugin_math
    if _plugin_math is None:
        src = os.path.join(HERE, "plugin_math_host.hip")
        L = C.CDLL(nb.build(PLUGIN_MATH, nb.hip_host_lib(src), [src] + nb.include_files(), "plugin_math_host"))
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
        L = po.declare(C.CDLL(build()))  # the oracle's own entry points, which pyoracle.Oracle's methods call
        h = C.c_void_p
        L.quadrotor_oracle_create.restype = h
        L.quadrotor_oracle_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int]
        L.quadrotor_terminal_cost.restype = C.c_float
        L.quadrotor_terminal_cost.argtypes = [h, _f32p]
        L.quadrotor_det_atan2.argtypes = [_f32p, _f32p, _f32p, C.c_int]
        L.quadrotor_quat_eval.argtypes = [C.c_int, _f32p, _f32p]
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
    """builds examples/quadrotor_model/quadrotor_model.hip on its own and loads it into the engine's registry with
    mppi_load_plugin; m is the mppi_generic_amd package"""
    return nb.load_plugin_model(m, "quadrotor", MODEL_SRC, MODEL_LIB)
