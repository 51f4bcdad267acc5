"""The CPU restatement of ARRobustCost (ar_robust_oracle.cpp) and the host build of the shipped class (robust_cost_host.hip) for
the tests: build helpers and ctypes loaders.

ar_robust_oracle.cpp is compiled together with the unchanged oracle/oracle_capi.cpp into ONE library, with the flags of
oracle/Makefile, exactly as tests/quadrotor_map_oracle/__init__.py builds its own: the handle is an oracle::Controller (the
oracle's ARNeuralNetModel + the restated cost) and every oracle_* entry point takes it, the Robust MPPI ones included.
"""
import ctypes as C
import os
import subprocess

import numpy as np

import pyoracle as po

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
ORACLE = os.path.join(REPO, "oracle")
LIB = os.path.join(HERE, "_build", "libar_robust_oracle.so")
HOST_LIB = os.path.join(HERE, "_build", "librobust_cost_host.so")
MODEL_SRC = os.path.join(REPO, "examples", "autorally_robust_model", "autorally_robust_model.hip")
MODEL_LIB = os.path.join(REPO, "examples", "_build", "libautorally_robust_model.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# oracle/Makefile's CXXFLAGS: -ffp-contract=off keeps det::fma() the only fused operation
CXXFLAGS = ["-O2", "-std=c++17", "-fPIC", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-Wall",
            "-Wno-unused-parameter"]
_f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
_i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
_lib = _host = None

CENSUS = ("below_threshold", "on_ramp", "saturated", "track_on", "track_off", "speed_from_map", "speed_from_param", "heading",
          "slip_below", "slip_ramp", "slip_saturated", "rolled", "max_cost")


def _include_files():
    return [os.path.join(d, f) for d, _, fs in os.walk(os.path.join(REPO, "include")) for f in fs]


def _stale(target, deps):
    return not os.path.exists(target) or any(os.path.getmtime(s) > os.path.getmtime(target) for s in deps)


def _compile(cmd, target, what):
    os.makedirs(os.path.dirname(target), exist_ok=True)
    r = subprocess.run(cmd + ["-o", target + ".tmp"], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(what + " build failed:\n" + r.stdout[-3000:] + r.stderr[-6000:])
    os.replace(target + ".tmp", target)


def build():
    src = os.path.join(HERE, "ar_robust_oracle.cpp")
    deps = [src, os.path.abspath(__file__)]
    deps += [os.path.join(ORACLE, f) for f in os.listdir(ORACLE) if f.endswith((".cpp", ".hpp"))]
    deps += [os.path.join(REPO, "include", "mppi_amd", f) for f in ("det_math.h", "model_params.h")]
    if _stale(LIB, deps):
        _compile([os.environ.get("CXX", "g++")] + CXXFLAGS + ["-I" + os.path.join(REPO, "include"), "-I" + ORACLE, "-shared",
                 os.path.join(ORACLE, "oracle_capi.cpp"), src], LIB, "AutoRally robust oracle")
    return LIB


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        h = C.c_void_p
        L.ar_robust_oracle_create.restype = h
        L.ar_robust_oracle_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int]
        L.ar_robust_set_costmap.argtypes = [h, _f32p, C.c_int, C.c_int]
        L.ar_robust_terms.argtypes = [h, _f32p, _f32p]
        L.ar_robust_census.argtypes = [h, _f32p, _f32p, C.c_int, C.c_int, _i32p]
        # the library holds oracle_capi.cpp too: its entry points get the declarations oracle/pyoracle.py gives its own copy
        for name, fn in list(vars(po.lib()).items()):
            if name.startswith("oracle_") and getattr(fn, "argtypes", None) is not None:
                mine = getattr(L, name)
                mine.argtypes, mine.restype = fn.argtypes, fn.restype
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
            if _stale(HOST_LIB, [src] + _include_files()):
                _compile([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC",
                          "-shared", "-Werror", "-I" + os.path.join(REPO, "include"), src], HOST_LIB, "robust_cost_host")
            L = C.CDLL(HOST_LIB)
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
    lib_ = m.load_library()
    if "autorally_nn_robust" in m.list_models():
        return lib_
    if _stale(MODEL_LIB, [MODEL_SRC] + _include_files()):
        _compile([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                  "-I" + os.path.join(REPO, "include"), MODEL_SRC], MODEL_LIB, "autorally_robust_model")
    assert lib_.mppi_load_plugin(MODEL_LIB.encode()) == m.MPPI_OK, lib_.mppi_last_error(None)
    return lib_
