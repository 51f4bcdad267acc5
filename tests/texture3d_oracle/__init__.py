"""The CPU restatement of the 3-D texture lookup and of QuadrotorVolumeCost (texture3d_oracle.cpp), and the host build of the
shipped helper, host class and cost (texture3d_host.hip), for the tests: build helpers and ctypes loaders.

texture3d_oracle.cpp includes tests/quadrotor_oracle/quadrotor_oracle.cpp (the dynamics and the quadratic cost, unchanged) and is
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
LIB = os.path.join(HERE, "_build", "libtexture3d_oracle.so")
HOST_LIB = os.path.join(HERE, "_build", "libtexture3d_host.so")
HOST_EXE = os.path.join(HERE, "_build", "texture3d_host_asan")
HOST_SRC = os.path.join(HERE, "texture3d_host.hip")
MODEL_SRC = os.path.join(REPO, "examples", "quadrotor_model", "quadrotor_volume_model.hip")
MODEL_LIB = os.path.join(REPO, "examples", "_build", "libquadrotor_volume_model.so")
_f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
_i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
_lib = _host = None

CLAMP, BORDER, WRAP = 0, 1, 2
LINEAR, POINT = 0, 1
IDENTITY_FRAME = np.array([0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 1, 1], np.float32)


def build():
    src = os.path.join(HERE, "texture3d_oracle.cpp")
    deps = [src, os.path.abspath(__file__), os.path.join(qo.HERE, "quadrotor_oracle.cpp")] + nb.oracle_files()
    return nb.build(LIB, nb.oracle_lib(src), deps, "texture3d oracle")


def lib():
    global _lib
    if _lib is None:
        L = po.declare(C.CDLL(build()))  # the oracle's own entry points, which pyoracle.Oracle's methods call
        h = C.c_void_p
        L.texture3d_oracle_query.argtypes = [_f32p, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, _f32p, _f32p, _f32p, C.c_int, C.c_int,
                                             _f32p]
        L.quadrotor_volume_oracle_create.restype = h
        L.quadrotor_volume_oracle_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int]
        L.quadrotor_volume_set_volume.argtypes = [h, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.quadrotor_volume_terms.argtypes = [h, _f32p, _f32p]
        L.quadrotor_volume_census.argtypes = [h, _f32p, _f32p, C.c_int, C.c_int, _i32p]
        L.quadrotor_terminal_cost.restype = C.c_float  # of the included quadrotor_oracle.cpp: the handle's own terminalCost
        L.quadrotor_terminal_cost.argtypes = [h, _f32p]
        _lib = L
    return _lib


def host():
    """the shipped helper, host class and cost built for the host (hipcc --cuda-host-only: no device pass, nothing of the GPU is
    touched when it is loaded)"""
    global _host
    if _host is None:
        L = C.CDLL(nb.build(HOST_LIB, nb.hip_host_lib(HOST_SRC, "-Werror"), [HOST_SRC] + nb.include_files(), "texture3d_host"))
        L.helper3d_query.argtypes = [_f32p, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, _f32p, _f32p, _f32p, C.c_int, C.c_int, C.c_int,
                                     _f32p]
        L.helper3d_wrap_z.restype = C.c_float
        L.helper3d_wrap_z.argtypes = [C.c_float, C.c_float]
        L.helper3d_modes_refused.argtypes = [_i32p, C.c_int, C.c_char_p, C.c_int]
        L.host3d_update_layer.argtypes = [C.c_int, _f32p, C.c_int, C.c_int]
        L.host3d_update_volume.argtypes = [_f32p, C.c_int]
        L.host3d_values.argtypes = [_f32p, C.c_int]
        L.host3d_dirty.argtypes = [_i32p, C.c_int]
        L.host3d_copy.argtypes = [np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS"), C.c_int]
        L.host3d_image.argtypes = [_f32p, C.c_int]
        L.host3d_query_image.argtypes = [_f32p, _f32p]
        L.volume_cost_default_params.argtypes = [C.c_void_p]
        L.volume_cost_set_params.argtypes = [C.c_void_p]
        L.volume_cost_set_volume.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.volume_cost_state_cost.restype = C.c_float
        L.volume_cost_state_cost.argtypes = [_f32p]
        L.volume_cost_terminal_cost.restype = C.c_float
        L.volume_cost_terminal_cost.argtypes = [_f32p]
        L.volume_cost_terms.argtypes = [_f32p, _f32p]
        _host = L
    return _host


def build_host_program():
    """texture3d_host.hip with its main(), host pass only, under the address and undefined-behaviour sanitizers: a stand-alone
    program that is run as a child process (nothing of it is loaded into Python)"""
    cmd = nb.hip_host(HOST_SRC, "-DTEXTURE3D_HOST_MAIN", "-Werror", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                      "-fno-sanitize-recover=all")
    return nb.build(HOST_EXE, cmd, [HOST_SRC] + nb.include_files(), "texture3d_host_asan")


def frame15(origin, rotations, resolution):
    """origin[3], rotations[9] row-major, resolution[3]: the "cost_volume_transform" blob"""
    return np.concatenate([np.asarray(origin, np.float32).reshape(3), np.asarray(rotations, np.float32).reshape(9),
                           np.asarray(resolution, np.float32).reshape(3)])


def _args(data, points, address_mode, filter_mode, border_color, frame):
    d = np.ascontiguousarray(data, np.float32)
    if d.ndim == 3:
        d = d[:, :, :, None]
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    modes = np.array(list(address_mode) + [filter_mode], np.int32)
    border = np.ascontiguousarray(border_color, np.float32)
    fr = np.ascontiguousarray(IDENTITY_FRAME if frame is None else frame, np.float32)
    assert modes.size == 4 and border.size == 4 and fr.size == 15
    return d, pts, modes, border, fr


def query(data, points, frame_kind=0, address_mode=(CLAMP, CLAMP, CLAMP), filter_mode=LINEAR, border_color=(0, 0, 0, 0), frame=None):
    """the restatement: data [d][h][w] or [d][h][w][ch], points [n][3] -> [n][ch]"""
    d, pts, modes, border, fr = _args(data, points, address_mode, filter_mode, border_color, frame)
    depth, h, w, ch = d.shape
    out = np.zeros((pts.shape[0], ch), np.float32)
    lib().texture3d_oracle_query(d.reshape(-1), w, h, depth, ch, modes, border, fr, pts.reshape(-1), pts.shape[0], frame_kind,
                                 out.reshape(-1))
    return out


def helper_query(data, points, frame_kind=0, address_mode=(CLAMP, CLAMP, CLAMP), filter_mode=LINEAR, border_color=(0, 0, 0, 0),
                 frame=None, batch=0):
    """the shipped helper's host form, same arguments; batch = 1, 3, 4: queryTextureAtWorldPoseBatch<batch>"""
    d, pts, modes, border, fr = _args(data, points, address_mode, filter_mode, border_color, frame)
    depth, h, w, ch = d.shape
    out = np.zeros((pts.shape[0], ch), np.float32)
    host().helper3d_query(d.reshape(-1), w, h, depth, ch, modes, border, fr, pts.reshape(-1), pts.shape[0], frame_kind, batch,
                          out.reshape(-1))
    return out


class QuadrotorVolumeOracle(po.Oracle):
    """pyoracle.Oracle on the restatement of QuadrotorDynamics + QuadrotorVolumeCost"""

    def __init__(self, K, T, D=1, dt=0.01, lambda_=1.0, alpha=0.0, num_iters=1):
        self.L = lib()
        self.h = self.L.quadrotor_volume_oracle_create(K, T, D, dt, lambda_, alpha, num_iters)
        self.S, self.C, self.O = 13, 4, 13
        self.K, self.T, self.D = K, T, D
        self.dt, self.lambda_, self.alpha, self.num_iters = dt, lambda_, alpha, num_iters

    def set_volume(self, values, frame):
        """values [depth][height][width] or None (no volume); frame: frame15(...)"""
        if values is None:
            self.L.quadrotor_volume_set_volume(self.h, None, 0, 0, 0, None)
            return
        v, f = np.ascontiguousarray(values, np.float32), np.ascontiguousarray(frame, np.float32)
        assert v.ndim == 3 and f.size == 15
        self.L.quadrotor_volume_set_volume(self.h, v.ctypes.data, v.shape[0], v.shape[1], v.shape[2], f.ctypes.data)

    def terms(self, s):
        """the volume's value at the position, the volume term, the quadratic part"""
        out = np.zeros(3, np.float32)
        self.L.quadrotor_volume_terms(self.h, np.ascontiguousarray(s, np.float32).reshape(-1), out)
        return out

    def terminal_cost(self, y):
        return float(self.L.quadrotor_terminal_cost(self.h, np.ascontiguousarray(y, np.float32).reshape(-1)))

    def inside(self, x0, samples):
        """[K][T] bool: is the output of step t of rollout k inside the volume on every axis (the border rule)"""
        v = np.ascontiguousarray(samples, np.float32).reshape(-1, self.T, 4)
        out = np.zeros(v.shape[0] * self.T, np.int32)
        self.L.quadrotor_volume_census(self.h, np.ascontiguousarray(x0, np.float32).reshape(-1), v.reshape(-1), v.shape[0], self.T, out)
        return out.reshape(v.shape[0], self.T).astype(bool)


class HostCost:
    """the shipped QuadrotorVolumeCost built for the host.  One object per process: the library holds one cost instance."""

    def __init__(self):
        self.L = host()
        self._volume = None

    def set_cost_params(self, p):
        self.L.volume_cost_set_params(C.byref(p))

    def set_volume(self, values, frame):
        if values is None:
            self._volume = None
            self.L.volume_cost_set_volume(None, 0, 0, 0, None)
            return
        v, f = np.ascontiguousarray(values, np.float32).copy(), np.ascontiguousarray(frame, np.float32)
        self._volume = v  # the class keeps the pointer
        self.L.volume_cost_set_volume(v.ctypes.data, v.shape[0], v.shape[1], v.shape[2], f.ctypes.data)

    def terms(self, s):
        out = np.zeros(3, np.float32)
        self.L.volume_cost_terms(np.ascontiguousarray(s, np.float32).reshape(-1), out)
        return out

    def state_cost(self, s):
        return np.float32(self.L.volume_cost_state_cost(np.ascontiguousarray(s, np.float32).reshape(-1)))

    def terminal_cost(self, s):
        return np.float32(self.L.volume_cost_terminal_cost(np.ascontiguousarray(s, np.float32).reshape(-1)))


def load_model(m):
    """builds examples/quadrotor_model/quadrotor_volume_model.hip on its own and loads it into the engine's registry with
    mppi_load_plugin (as quadrotor_oracle.load_model does for "quadrotor"); m is the mppi_generic_amd package"""
    return nb.load_plugin_model(m, "quadrotor_volume", MODEL_SRC, MODEL_LIB)
