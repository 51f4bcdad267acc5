"""Closing a controller releases every device, pinned and mapped allocation it made: the process-wide count of live
allocations (mppi_debug_live_allocations) rises while the controller is in use and is back at its starting value, count and
bytes, once it is closed.  One case per way a handle allocates — creation, the reallocation sites, the model's blobs and the
temporaries of single calls."""
import ctypes as C
import gc

import numpy as np
import pytest

import mppi_generic_amd as m
from common import SEED, autorally_cfg, cartpole_cfg, di_cfg, host_noise, make_engine

pytestmark = pytest.mark.gpu

K, T = 256, 20


def _live(lib):
    n, b = C.c_int64(), C.c_int64()
    assert lib.mppi_debug_live_allocations(C.byref(n), C.byref(b)) == m.MPPI_OK
    return n.value, b.value


def _released(lib, use):
    """use() creates one controller and drives it"""
    gc.collect()  # controllers of earlier tests that only a collection frees
    before = _live(lib)
    eng = use()
    during = _live(lib)
    assert during[0] > before[0] and during[1] > before[1], (before, during)
    eng.close()
    assert _live(lib) == before


def _control(eng, x0, n=2):
    for _ in range(n):
        eng.computeControl(x0, 1)
    eng.getControlSeq()
    eng.getTargetStateSeq()
    return eng


def _robust(cfg):
    eng = m.RobustMPPIController(cfg["model"], cfg["K"], cfg["T"], cfg["dt"], cfg["lambda_"], cfg["alpha"], 1, seed=SEED)
    if cfg["dyn"] is not None:
        eng.setDynamicsParams(cfg["dyn"])
    eng.setCostParams(cfg["cost"])
    for name, blob in cfg.get("blobs", {}).items():
        eng.setModelBlob(name, blob)
    if cfg["ranges"] is not None:
        eng.setControlRanges(cfg["ranges"])
    eng.setSamplingParams(cfg["std_dev"], [0.2, 0.1])
    eng.setRMPPIParams(500.0, 9, 32)
    x = cfg["x0"].copy()
    for i in range(2):
        eng.updateImportanceSamplingControl(x, 1)  # candidate buffers
        g = np.random.default_rng(i).uniform(-0.3, 0.3, (cfg["T"], eng.STATE_DIM, eng.CONTROL_DIM)).astype(np.float32)
        eng.setFeedbackGains(g)
        eng.computeControl(x, 1)
    return eng


def _vanilla():
    cfg = cartpole_cfg(K=K, T=T)
    eng = _control(make_engine(cfg), cfg["x0"])  # own stream: split hand-over, and the BAR inbox where the device has one
    eng.modelStep(cfg["x0"], np.zeros(1, np.float32))
    return eng


def _colored_tsallis():
    cfg = cartpole_cfg(K=K, T=T)
    cfg["colored"] = ([1.0], 0.97, 0.0)
    eng = make_engine(cfg)
    eng.setColoredMPPIParams(gamma=400.0, r_exp=1.7)
    return _control(eng, cfg["x0"])


def _tube():
    cfg = di_cfg(K=K, T=T, tube=True)
    return _control(make_engine(cfg), cfg["x0"])


def _robust_di():
    return _robust(di_cfg(K=2 * K, T=T, tube=True))  # 9 candidates x 32 samples need K >= 288


def _robust_autorally():
    cfg = autorally_cfg(K=2 * K, T=T)
    cfg["D"] = 2
    return _robust(cfg)


def _reference_order():
    cfg = cartpole_cfg(K=K, T=T)
    eng = make_engine(cfg)
    eng.setReductionMode(m.MPPI_REDUCTION_REFERENCE_ORDER)
    return _control(eng, cfg["x0"])


def _injected_noise():
    cfg = cartpole_cfg(K=K, T=T)
    eng = make_engine(cfg)
    eng.injectNoise(host_noise(1, K, T, 1))
    eng.computeControl(cfg["x0"], 1)
    eng.injectNoise(host_noise(3, K, T, 1))
    eng.computeControl(cfg["x0"], 1)
    eng.sampleNoise()
    eng.setIndependentNoise(True)
    return _control(eng, cfg["x0"])


def _time_specific_std_dev():
    cfg = cartpole_cfg(K=K, T=T)
    eng = make_engine(cfg)
    eng.setTimeSpecificStdDev(np.linspace(1.0, 5.0, T, dtype=np.float32).reshape(T, 1))
    return _control(eng, cfg["x0"])


def _rocrand():
    cfg = cartpole_cfg(K=K, T=T)
    return _control(make_engine(cfg, noise_source=2), cfg["x0"])  # MPPI_NOISE_ROCRAND_HOST


def _choose_kernel():
    cfg = cartpole_cfg(K=K, T=T)
    eng = make_engine(cfg)
    eng.uploadState(cfg["x0"])
    eng.chooseAppropriateKernel(2)
    return eng


def _p2p_mailbox():
    eng = make_engine(cartpole_cfg(K=K, T=T), force_exchange=True)
    eng.p2pMailboxHandle()
    return eng


CASES = [_vanilla, _colored_tsallis, _tube, _robust_di, _robust_autorally, _reference_order, _injected_noise,
         _time_specific_std_dev, _rocrand, _choose_kernel, _p2p_mailbox]


@pytest.mark.parametrize("use", CASES, ids=[c.__name__[1:] for c in CASES])
def test_closing_a_controller_releases_its_allocations(gpu, lib, use):
    _released(lib, use)


def test_long_horizon_rows_and_finalize_scratch_in_hbm(gpu, lib, monkeypatch):
    monkeypatch.setenv("MPPI_AMD_ROWS_IN_HBM", "1")  # both read at create
    monkeypatch.setenv("MPPI_AMD_FINALIZE_SCRATCH", "1")
    cfg = cartpole_cfg(K=K, T=1000)
    _released(lib, lambda: _control(make_engine(cfg), cfg["x0"]))


def test_callers_stream(gpu, lib):
    hip = C.CDLL("libamdhip64.so")
    s = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(s)) == 0
    try:
        cfg = cartpole_cfg(K=K, T=T)
        _released(lib, lambda: _control(make_engine(cfg, stream=s.value), cfg["x0"]))
        assert hip.hipStreamSynchronize(s) == 0  # the handle left the caller's stream alive
    finally:
        hip.hipStreamDestroy(s)
