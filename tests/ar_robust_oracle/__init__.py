"""The CPU restatement of ARRobustCost (ar_robust_oracle.cpp) and the host build of the shipped class (robust_cost_host.hip) for
the tests: build helpers and ctypes loaders.

ar_robust_oracle.cpp is compiled together with the unchanged oracle/oracle_capi.cpp into ONE library (tests/native_build.py:
oracle_lib, the flags of oracle/Makefile): the handle is an oracle::Controller (the
oracle's ARNeuralNetModel + the restated cost) and every oracle_* entry point takes it, the Robust MPPI ones included.
"""
import ctypes as C
import os

import numpy as np

import native_build as nb
import pyoracle as po

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(HERE, "_build", "libar_robust_oracle.so")
HOST_LIB = os.path.join(HERE, "_build", "librobust_cost_host.so")
MODEL_SRC = os.path.join(REPO, "examples", "autorally_robust_model", "autorally_robust_model.hip")
MODEL_LIB = os.path.join(REPO, "examples", "_build", "libautorally_robust_model.so")
_f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
_i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
_lib = _host = None

CENSUS = ("below_threshold", "on_ramp", "saturated", "track_on", "track_off", "speed_from_map", "speed_from_param", "heading",
          "slip_below", "slip_ramp", "slip_saturated", "rolled", "max_cost")


def build():
    src = os.path.join(HERE, "ar_robust_oracle.cpp")
    return nb.build(LIB, nb.oracle_lib(src), [src, os.path.abspath(__file__)] + nb.oracle_files(), "AutoRally robust oracle")


def lib():
    global _lib
    if _lib is None:
        L = po.declare(C.CDLL(build()))  # the oracle's own entry points, the Robust MPPI ones included
        h = C.c_void_p
        L.ar_robust_oracle_create.restype = h
        L.ar_robust_oracle_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int]
        L.ar_robust_set_costmap.argtypes = [h, _f32p, C.c_int, C.c_int]
        L.ar_robust_terms.argtypes = [h, _f32p, _f32p]
        L.ar_robust_census.argtypes = [h, _f32p, _f32p, C.c_int, C.c_int, _i32p]
        _lib = L
    return _lib


def interleave(channels):
    """four [height][width] channels -> [height][width][4] texels"""
    return np.ascontiguousarray(np.stack([np.asarray(c, np.float32) for c in channels], axis=-1))


def _aligned(texels):
    """a 16-byte aligned, C-contiguous float32 copy (the class loads a texel as one 16-byte value)"""
    t = np.asarray(texels, np.float32)
    assert t.ndim == 3 and t.shape[2] == 4
    raw = np.zeros(t.size + 4, np.float32)
    off = (-raw.ctypes.data % 16) // 4
    out = raw[off:off + t.size].reshape(t.shape)
    out[...] = t
    assert out.ctypes.data % 16 == 0
    return out


class ARRobustOracle(po.Oracle):
    """pyoracle.Oracle on the oracle's ARNeuralNetModel + the restatement of ARRobustCost"""

    def __init__(self, K, T, D=1, dt=0.02, lambda_=1.0, alpha=0.0, num_iters=1):
        self.L = lib()
        self.h = self.L.ar_robust_oracle_create(K, T, D, dt, lambda_, alpha, num_iters)
        self.S, self.C, self.O = 7, 2, 8
        self.K, self.T, self.D = K, T, D
        self.dt, self.lambda_, self.alpha, self.num_iters = dt, lambda_, alpha, num_iters

    def set_blob(self, name, array):
        if name == "costmap":
            t = np.ascontiguousarray(array, np.float32)
            assert t.ndim == 3 and t.shape[2] == 4
            self.L.ar_robust_set_costmap(self.h, t.reshape(-1), t.shape[0], t.shape[1])
        else:
            super().set_blob(name, array)

    def terms(self, s):
        """stabilizing cost, constraint, track, speed, heading terms, costmap cost"""
        out = np.zeros(6, np.float32)
        self.L.ar_robust_terms(self.h, np.ascontiguousarray(s, np.float32).reshape(-1), out)
        return out

    def cost(self, s, t=0):
        c = C.c_int(0)
        v = self.L.oracle_state_cost(self.h, np.ascontiguousarray(s, np.float32).reshape(-1), t, C.byref(c))
        assert c.value == 0  # this cost never writes the crash flag
        return np.float32(v)

    def census(self, x0, samples):
        """branch counts over all rollout-steps of the clamped samples [K][T][2] from x0, by the names of CENSUS"""
        v = np.ascontiguousarray(samples, np.float32).reshape(-1, self.T, 2)
        counts = np.zeros(len(CENSUS), np.int32)
        self.L.ar_robust_census(self.h, np.ascontiguousarray(x0, np.float32).reshape(-1), v.reshape(-1), v.shape[0], self.T, counts)
        return dict(zip(CENSUS, counts.tolist()))


class HostCost:
    """the shipped ARRobustCost built for the host (robust_cost_host.hip through hipcc --cuda-host-only: no device pass, nothing
    of the GPU is touched when it is loaded).  One object per process: the library holds one cost instance."""

    def __init__(self):
        global _host
        if _host is None:
            src = os.path.join(HERE, "robust_cost_host.hip")
            L = C.CDLL(nb.build(HOST_LIB, nb.hip_host_lib(src, "-Werror"), [src] + nb.include_files(), "robust_cost_host"))
            L.robust_cost_default_params.argtypes = [C.c_void_p]
            L.robust_cost_field_offsets.argtypes = [_i32p, _i32p]
            L.robust_cost_set_params.argtypes = [C.c_void_p]
            L.robust_cost_set_costmap.argtypes = [C.c_void_p, C.c_int, C.c_int]
            L.robust_cost_state_cost.restype = C.c_float
            L.robust_cost_state_cost.argtypes = [_f32p, C.c_int, C.POINTER(C.c_int)]
            L.robust_cost_terms.argtypes = [_f32p, _f32p]
            L.robust_cost_texel_index.argtypes = [C.c_float, C.c_float]
            L.robust_cost_max_cost_value.restype = C.c_float
            _host = L
        self.L = _host
        self._map = None

    def set_cost_params(self, p):
        self.L.robust_cost_set_params(C.byref(p))

    def set_costmap(self, texels):
        self._map = _aligned(texels)  # the class keeps the pointer
        self.L.robust_cost_set_costmap(self._map.ctypes.data, self._map.shape[0], self._map.shape[1])

    def terms(self, s):
        """(stabilizing cost, costmap cost)"""
        out = np.zeros(2, np.float32)
        self.L.robust_cost_terms(np.ascontiguousarray(s, np.float32).reshape(-1), out)
        return out

    def stabilizing(self, s):
        """getStabilizingCost alone (it reads no map)"""
        out = np.zeros(2, np.float32)
        if self._map is None:
            self.set_costmap(np.zeros((1, 1, 4), np.float32))
        self.L.robust_cost_terms(np.ascontiguousarray(s, np.float32).reshape(-1), out)
        return out[0]

    def texel_index(self, x, y):
        return self.L.robust_cost_texel_index(x, y)

    def cost(self, s, t=0):
        c = C.c_int(0)
        v = self.L.robust_cost_state_cost(np.ascontiguousarray(s, np.float32).reshape(-1), t, C.byref(c))
        assert c.value == 0
        return np.float32(v)


def load_model(m):
    """builds examples/autorally_robust_model/autorally_robust_model.hip on its own and loads it into the engine's registry with
    mppi_load_plugin; m is the mppi_generic_amd package"""
    return nb.load_plugin_model(m, "autorally_nn_robust", MODEL_SRC, MODEL_LIB)
