"""The CPU restatement of QuadrotorMapCost (quadrotor_map_oracle.cpp) and the host build of the shipped class
(map_cost_host.hip) for the tests: build helpers and ctypes loaders.

quadrotor_map_oracle.cpp includes tests/quadrotor_oracle/quadrotor_oracle.cpp (the dynamics restatement, unchanged) and is
compiled together with the unchanged oracle/oracle_capi.cpp into ONE library (tests/native_build.py: oracle_lib, the flags of
oracle/Makefile): the handle is an oracle::Controller and every oracle_* entry point takes it.
"""
import ctypes as C
import os

import numpy as np

import native_build as nb
import pyoracle as po
import quadrotor_oracle as qo

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(HERE, "_build", "libquadrotor_map_oracle.so")
HOST_LIB = os.path.join(HERE, "_build", "libmap_cost_host.so")
MODEL_SRC = os.path.join(REPO, "examples", "quadrotor_model", "quadrotor_map_model.hip")
MODEL_LIB = os.path.join(REPO, "examples", "_build", "libquadrotor_map_model.so")
_f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
_i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
_lib = _host = None


def build():
    src = os.path.join(HERE, "quadrotor_map_oracle.cpp")
    deps = [src, os.path.abspath(__file__), os.path.join(qo.HERE, "quadrotor_oracle.cpp")] + nb.oracle_files()
    return nb.build(LIB, nb.oracle_lib(src), deps, "quadrotor map oracle")


def lib():
    global _lib
    if _lib is None:
        L = po.declare(C.CDLL(build()))  # the oracle's own entry points, which pyoracle.Oracle's methods call
        h = C.c_void_p
        L.quadrotor_map_oracle_create.restype = h
        L.quadrotor_map_oracle_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int]
        L.quadrotor_map_set_costmap.argtypes = [h, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.quadrotor_map_terms.argtypes = [h, _f32p, _f32p]
        L.quadrotor_map_census.argtypes = [h, _f32p, _f32p, C.c_int, C.c_int, _i32p, _i32p]
        _lib = L
    return _lib


def frame15(origin, rotations, resolution):
    """the "costmap_transform" blob: origin[3], rotations[9] row-major, resolution[3]"""
    return np.concatenate([np.asarray(origin, np.float32).reshape(3), np.asarray(rotations, np.float32).reshape(9),
                           np.asarray(resolution, np.float32).reshape(3)])


class QuadrotorMapOracle(po.Oracle):
    """pyoracle.Oracle on the restatement of QuadrotorDynamics + QuadrotorMapCost"""

    def __init__(self, K, T, D=1, dt=0.01, lambda_=1.0, alpha=0.0, num_iters=1):
        self.L = lib()
        self.h = self.L.quadrotor_map_oracle_create(K, T, D, dt, lambda_, alpha, num_iters)
        self.S, self.C, self.O = 13, 4, 13
        self.K, self.T, self.D = K, T, D
        self.dt, self.lambda_, self.alpha, self.num_iters = dt, lambda_, alpha, num_iters

    def set_costmap(self, values, frame):
        """values [height][width] or None (no map); frame: frame15(...)"""
        if values is None:
            self.L.quadrotor_map_set_costmap(self.h, None, 0, 0, None)
            return
        v, f = np.ascontiguousarray(values, np.float32), np.ascontiguousarray(frame, np.float32)
        assert v.ndim == 2 and f.size == 15
        self.L.quadrotor_map_set_costmap(self.h, v.ctypes.data, v.shape[0], v.shape[1], f.ctypes.data)

    def terms(self, s):
        """costmap, gate side, height, heading, speed, attitude, waypoint terms, distance to the waypoint"""
        out = np.zeros(8, np.float32)
        self.L.quadrotor_map_terms(self.h, np.ascontiguousarray(s, np.float32).reshape(-1), out)
        return out

    def state_cost_crash(self, s, crash=0, t=0):
        """(cost, crash flag afterwards) of one evaluation that starts with the given flag"""
        c = C.c_int(crash)
        cost = self.L.oracle_state_cost(self.h, np.ascontiguousarray(s, np.float32).reshape(-1), t, C.byref(c))
        return np.float32(cost), c.value

    def census(self, x0, samples):
        """branch counts over all rollout-steps of the clamped samples [K][T][4] from x0, and each rollout's first crash step:
        (dict, first_crash[K])"""
        v = np.ascontiguousarray(samples, np.float32).reshape(-1, self.T, 4)
        counts, first = np.zeros(7, np.int32), np.zeros(v.shape[0], np.int32)
        self.L.quadrotor_map_census(self.h, np.ascontiguousarray(x0, np.float32).reshape(-1), v.reshape(-1), v.shape[0], self.T,
                                    counts, first)
        names = ("left_map", "off_track", "gate_hit", "gate_passed", "heading_on", "heading_off", "height_400")
        return dict(zip(names, counts.tolist())), first


class HostCost:
    """the shipped QuadrotorMapCost built for the host (map_cost_host.hip through hipcc --cuda-host-only: no device pass, nothing
    of the GPU is touched when it is loaded).  One object per process: the library holds one cost instance."""

    def __init__(self):
        global _host
        if _host is None:
            src = os.path.join(HERE, "map_cost_host.hip")
            L = C.CDLL(nb.build(HOST_LIB, nb.hip_host_lib(src, "-Werror"), [src] + nb.include_files(), "map_cost_host"))
            L.map_cost_default_params.argtypes = [C.c_void_p]
            L.map_cost_field_offsets.argtypes = [_i32p, _i32p]
            L.map_cost_update_waypoint.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float]
            L.map_cost_update_gate.argtypes = [C.c_void_p, _f32p]
            L.map_cost_set_params.argtypes = [C.c_void_p]
            L.map_cost_set_costmap.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
            L.map_cost_state_cost.restype = C.c_float
            L.map_cost_state_cost.argtypes = [_f32p, C.c_int, C.POINTER(C.c_int)]
            L.map_cost_terminal_cost.restype = C.c_float
            L.map_cost_terminal_cost.argtypes = [_f32p]
            L.map_cost_terms.argtypes = [_f32p, _f32p]
            L.map_cost_max_cost_value.restype = C.c_float
            _host = L
        self.L = _host
        self._map = None

    def set_cost_params(self, p):
        self.L.map_cost_set_params(C.byref(p))

    def set_costmap(self, values, frame):
        if values is None:
            self._map = None
            self.L.map_cost_set_costmap(None, 0, 0, None)
            return
        v, f = np.ascontiguousarray(values, np.float32).copy(), np.ascontiguousarray(frame, np.float32)
        self._map = v  # the class keeps the pointer
        self.L.map_cost_set_costmap(v.ctypes.data, v.shape[0], v.shape[1], f.ctypes.data)

    def terms(self, s):
        out = np.zeros(8, np.float32)
        self.L.map_cost_terms(np.ascontiguousarray(s, np.float32).reshape(-1), out)
        return out

    def state_cost_crash(self, s, crash=0, t=0):
        c = C.c_int(crash)
        cost = self.L.map_cost_state_cost(np.ascontiguousarray(s, np.float32).reshape(-1), t, C.byref(c))
        return np.float32(cost), c.value

    def terminal_cost(self, s):
        return self.L.map_cost_terminal_cost(np.ascontiguousarray(s, np.float32).reshape(-1))


def load_model(m):
    """builds examples/quadrotor_model/quadrotor_map_model.hip on its own and loads it into the engine's registry with
    mppi_load_plugin (as quadrotor_oracle.load_model does for "quadrotor"); m is the mppi_generic_amd package"""
    return nb.load_plugin_model(m, "quadrotor_map", MODEL_SRC, MODEL_LIB)
