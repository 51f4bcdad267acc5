"""The host build of the shipped computeGrad methods (linearize_host.hip) for the tests: ctypes loader over a library
tests/native_build.py builds: hipcc for the host alone (no device pass, nothing of the GPU is touched when it is loaded)."""
import ctypes as C
import os

import numpy as np

import native_build as nb

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB = os.path.join(HERE, "_build", "liblinearize_host.so")
_f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
_lib = None

MODELS = {"cartpole": 0, "double_integrator": 1, "racer_dubins": 2, "quadrotor": 3, "autorally_nn": 4}
DIMS = {"cartpole": (4, 1), "double_integrator": (4, 2), "racer_dubins": (7, 2), "quadrotor": (13, 4), "autorally_nn": (7, 2)}
TRAIT_CLASSES = ("CartpoleDynamics", "DoubleIntegratorDynamics", "RacerDubins", "QuadrotorDynamics", "NeuralNetModel",
                 "NeuralNetModelMFMA", "NeuralNetModelWave", "RacerDubinsElevation", "BicycleSlipLSTM")


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(HERE, "linearize_host.hip")
        L = C.CDLL(nb.build(HOST_LIB, nb.hip_host_lib(src), [src] + nb.include_files(), "linearize_host"))
        L.linearize_host_eval.argtypes = [C.c_int, _f32p, _f32p, _f32p, _f32p, C.c_int, _f32p, _f32p, C.POINTER(C.c_int)]
        L.linearize_host_traits.restype = C.c_uint
        _lib = L
    return _lib


def host_grad(model, x, u, params=None, weights=None):
    """(A (n, S, S), B (n, S, C), returned) of the shipped class built for the host, at the points x (n, S), u (n, C)"""
    S, Cd = DIMS[model]
    x = np.ascontiguousarray(x, np.float32).reshape(-1, S)
    u = np.ascontiguousarray(u, np.float32).reshape(-1, Cd)
    n = x.shape[0]
    assert u.shape[0] == n
    A = np.full((n, S, S), np.nan, np.float32)
    B = np.full((n, S, Cd), np.nan, np.float32)
    p = np.ascontiguousarray(params if params is not None else np.zeros(4), np.float32)
    w = np.ascontiguousarray(weights if weights is not None else np.zeros(1), np.float32)
    ret = C.c_int(-1)
    dims = lib().linearize_host_eval(MODELS[model], p, w, x.reshape(-1), u.reshape(-1), n, A.reshape(-1), B.reshape(-1), C.byref(ret))
    assert dims == S * 100 + Cd, dims
    return A, B, bool(ret.value)


def traits():
    """{class name: (declares computeGrad, in the wave-per-point form)}"""
    bits = lib().linearize_host_traits()
    return {name: (bool(bits >> i & 1), bool(bits >> (16 + i) & 1)) for i, name in enumerate(TRAIT_CLASSES)}
