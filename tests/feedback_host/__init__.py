"""The host build of the DDP backward pass (feedback_host.hip: include/mppi_amd/feedback_controllers/ddp_backward.hpp) for the
tests: ctypes loader over a library tests/native_build.py builds: hipcc for the host alone (no device pass, nothing
of the GPU is touched when it is loaded)."""
import ctypes as C
import os

import numpy as np

import native_build as nb

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB = os.path.join(HERE, "_build", "libfeedback_host.so")
_f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
_lib = None


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(HERE, "feedback_host.hip")
        L = C.CDLL(nb.build(HOST_LIB, nb.hip_host_lib(src), [src] + nb.include_files(), "feedback_host"))
        L.feedback_host_backward.argtypes = [C.c_int, _f32p, _f32p, _f32p, _f32p, _f32p, C.c_float, C.c_int, _f32p, C.POINTER(C.c_int)]
        _lib = L
    return _lib


def host_gains(A, B, dt, Q=None, R=None, Qf=None, out=None):
    """(gains (T, S, C), ok, failing step) of the host build over A (T, S, S), B (T, S, C) float32; None weights are identities
    (the DDPParams default); `out`: the array the rows are written into (default: one filled with NaN)"""
    A = np.ascontiguousarray(A, np.float32)
    B = np.ascontiguousarray(B, np.float32)
    T, S, Cd = B.shape
    assert A.shape == (T, S, S)
    Q = np.ascontiguousarray(np.eye(S) if Q is None else Q, np.float32)
    R = np.ascontiguousarray(np.eye(Cd) if R is None else R, np.float32)
    Qf = np.ascontiguousarray(np.eye(S) if Qf is None else Qf, np.float32)
    assert Q.shape == (S, S) and R.shape == (Cd, Cd) and Qf.shape == (S, S)
    g = np.full((T, S, Cd), np.nan, np.float32) if out is None else out
    assert g.shape == (T, S, Cd) and g.dtype == np.float32 and g.flags.c_contiguous
    step = C.c_int(-7)
    ok = lib().feedback_host_backward(S * 100 + Cd, A.reshape(-1), B.reshape(-1), Q.reshape(-1), R.reshape(-1), Qf.reshape(-1),
                                      float(dt), T, g.reshape(-1), C.byref(step))
    assert ok in (0, 1), ok
    return g, bool(ok), step.value
