"""What mppi_set_model_blob and mppi_set_lstm_initial_state refuse, and with which words: one row per branch of ModelT::setBlob and
ModelT::setLSTMInitialState (engine/model_blobs.hpp holds the helpers they are written on), each pinned to its exact status and
its exact mppi_last_error text, on the smallest controller every model accepts (K = 64, T = 4).  A refusal leaves the handle as
it was, so the rows of a model share one handle.  Then one accepted blob set per map kind — elevation map, normals map (which
inherits the elevation map's frame: the suspension model is given "elevation_map_transform" alone), the one- and the
four-channel "costmap" and the cost texture — run against its oracle: trajectory costs 0 ulp, u* within 1e-5.

Everything here needs a handle, and mppi_create gives none without a HIP device: the file is GPU only."""
import ctypes as C

import numpy as np
import pytest

import mppi_generic_amd as m
from common import U_TOL, autorally_cfg, bicycle_lstm_cfg, cartpole_cfg, host_noise, make_engine, make_oracle, ulp_diff
from racer_cfgs import elevation_cfg, steering_cfg, suspension_cfg, uncertainty_cfg
from test_ar_robust_cost import make_robust_oracle, robust_cfg
from test_quadrotor_map_cost import make_map_oracle, map_cfg, nominal_control

K, T = 64, 4
PLUGIN_MODELS = ("quadrotor_map", "autorally_nn_robust")  # registered from examples/ only


def _without(cfg, *names):
    return dict(cfg, blobs={k: v for k, v in cfg["blobs"].items() if k not in names})


NETWORKS = ("mean_lstm_weights", "mean_lstm_output_weights", "unc_lstm_weights", "unc_lstm_output_weights")
CONFIGS = {
    "cartpole": lambda: cartpole_cfg(K=K, T=T),
    "autorally_nn": lambda: autorally_cfg(K=K, T=T),
    "bicycle_slip_lstm": lambda: bicycle_lstm_cfg(K=K, T=T),
    "bicycle_slip_lstm/no-weights": lambda: _without(bicycle_lstm_cfg(K=K, T=T), "lstm_weights", "lstm_output_weights"),
    "racer_dubins_elevation": lambda: elevation_cfg(K=K, T=T),
    "racer_dubins_elevation_lstm_steering": lambda: steering_cfg(K=K, T=T),
    "racer_dubins_elevation_suspension": lambda: suspension_cfg(K=K, T=T),
    "racer_dubins_elevation_lstm_unc": lambda: uncertainty_cfg(K=K, T=T),
    "racer_dubins_elevation_lstm_unc/no-weights": lambda: _without(uncertainty_cfg(K=K, T=T), *NETWORKS),
    "autorally_nn_robust": lambda: robust_cfg(K=K, T=T),
    "quadrotor_map": lambda: map_cfg(K=K, T=T, with_map=False),
}


@pytest.fixture(scope="module")
def plugins(lib):
    """"quadrotor_map" and "autorally_nn_robust" are loaded the way tests/test_quadrotor_map_cost.py and
    tests/test_ar_robust_cost.py load them, and what this module registered leaves the process-wide registry with it: the
    kernel-form files that run later enumerate the registry and want a configuration builder for every name in it"""
    import ar_robust_oracle as ar
    import quadrotor_map_oracle as qm
    before = set(m.list_models())
    qm.load_model(m)
    ar.load_model(m)
    yield
    for name in PLUGIN_MODELS:
        if name not in before:
            assert lib.mppi_unregister_model(name.encode(), m.MPPI_SAMPLER_GAUSSIAN) == m.MPPI_OK


@pytest.fixture(scope="module")
def handle(gpu, plugins):
    made = {}

    def get(key):
        if key not in made:
            made[key] = make_engine(CONFIGS[key]())
        return made[key]
    yield get
    for eng in made.values():
        eng.close()


def _last_error(eng):
    return (eng._lib.mppi_last_error(eng._h) or b"").decode()


def _set_blob(eng, name, array, count=None, dims=None):
    a = np.ascontiguousarray(array, np.float32)
    dims = a.shape if dims is None else dims
    st = eng._lib.mppi_set_model_blob(eng._h, name.encode(), a.reshape(-1), a.size if count is None else count,
                                      (C.c_int * len(dims))(*dims), len(dims))
    return st, _last_error(eng)


def _set_state(eng, hidden, cell):
    st = eng._lib.mppi_set_lstm_initial_state(eng._h, np.ascontiguousarray(hidden, np.float32), np.ascontiguousarray(cell, np.float32))
    return st, _last_error(eng)


def expected(name, n, got):
    return "%s: expected %d floats, got %d" % (name, n, got)


MAP_2 = "%s: dims must be {height, width} with height*width == count"
MAP_4 = "%s: dims must be {height, width, 4} with height*width*4 == count"
COSTMAP_4 = ("costmap: this model's cost reads 4 channels: dims must be {height, width, 4} (interleaved texels) with "
             "height*width*4 == count")
FRAME = "%s: expected 15 floats (origin[3], rotations[9], resolution[3])"
STRUCTURE = "%s: expected {H, H + inputs, ..., outputs} with "
UNC, UNC_BARE = "racer_dubins_elevation_lstm_unc", "racer_dubins_elevation_lstm_unc/no-weights"
INVALID, STATE = m.MPPI_ERR_INVALID_ARG, m.MPPI_ERR_STATE

# (handle, blob, keyword arguments of _set_blob, status, mppi_last_error)
BLOB_ROWS = [
    # ---- "expected N floats, got M": the network parameter blobs and the mean / uncertainty networks' states
    ("autorally_nn", "dynamics_weights", dict(array=np.zeros(1411)), INVALID, expected("dynamics_weights", 1412, 1411)),
    ("bicycle_slip_lstm", "lstm_weights", dict(array=np.zeros(1503)), INVALID, expected("lstm_weights", 1504, 1503)),
    ("bicycle_slip_lstm", "lstm_output_weights", dict(array=np.zeros(869)), INVALID, expected("lstm_output_weights", 868, 869)),
    (UNC, "mean_lstm_weights", dict(array=np.zeros(279)), INVALID, expected("mean_lstm_weights", 280, 279)),
    (UNC, "mean_lstm_output_weights", dict(array=np.zeros(383)), INVALID, expected("mean_lstm_output_weights", 382, 383)),
    (UNC, "unc_lstm_weights", dict(array=np.zeros(295)), INVALID, expected("unc_lstm_weights", 296, 295)),
    (UNC, "unc_lstm_output_weights", dict(array=np.zeros(466)), INVALID, expected("unc_lstm_output_weights", 465, 466)),
    (UNC, "mean_lstm_state", dict(array=np.zeros(7)), INVALID, expected("mean_lstm_state", 8, 7)),
    (UNC, "unc_lstm_state", dict(array=np.zeros(9)), INVALID, expected("unc_lstm_state", 8, 9)),
    # ---- a state before its network's weights; a wrong count is refused first
    (UNC_BARE, "mean_lstm_state", dict(array=np.zeros(8)), STATE, "set the network's weights before its state"),
    (UNC_BARE, "unc_lstm_state", dict(array=np.zeros(8)), STATE, "set the network's weights before its state"),
    (UNC_BARE, "mean_lstm_state", dict(array=np.zeros(7)), INVALID, expected("mean_lstm_state", 8, 7)),
    # ---- a network shape that is none
    ("racer_dubins_elevation_lstm_steering", "lstm_structure", dict(array=[4.0]), INVALID,
     STRUCTURE % "lstm_structure" + "at least one output-network layer"),
    (UNC, "mean_lstm_structure", dict(array=[4.0]), INVALID,
     STRUCTURE % "mean_lstm_structure" + "the model's input / output sizes (12 -> 2, 13 -> 5)"),
    (UNC, "unc_lstm_structure", dict(array=[4.0, 17.0, 4.0]), INVALID,
     STRUCTURE % "unc_lstm_structure" + "the model's input / output sizes (12 -> 2, 13 -> 5)"),
    # ---- maps: the number of dims, a dim that is not positive, a product that is not the count, the channel count
    ("racer_dubins_elevation", "elevation_map", dict(array=np.zeros((9, 7, 1))), INVALID, MAP_2 % "elevation_map"),
    ("racer_dubins_elevation", "elevation_map", dict(array=np.zeros((9, 7)), dims=(9, 0)), INVALID, MAP_2 % "elevation_map"),
    ("racer_dubins_elevation", "elevation_map", dict(array=np.zeros((9, 7)), count=62), INVALID, MAP_2 % "elevation_map"),
    ("racer_dubins_elevation_suspension", "normals_map", dict(array=np.zeros((9, 7))), INVALID, MAP_4 % "normals_map"),
    ("racer_dubins_elevation_suspension", "normals_map", dict(array=np.zeros((9, 7, 3))), INVALID, MAP_4 % "normals_map"),
    ("racer_dubins_elevation_suspension", "normals_map", dict(array=np.zeros((9, 7, 4)), dims=(0, 7, 4)), INVALID,
     MAP_4 % "normals_map"),
    ("racer_dubins_elevation_suspension", "normals_map", dict(array=np.zeros((9, 7, 4)), count=251), INVALID, MAP_4 % "normals_map"),
    ("autorally_nn", "costmap", dict(array=np.zeros((9, 7, 4))), INVALID, MAP_2 % "costmap"),
    ("autorally_nn", "costmap", dict(array=np.zeros((9, 7)), dims=(7, 8)), INVALID, MAP_2 % "costmap"),
    ("autorally_nn_robust", "costmap", dict(array=np.zeros((9, 7))), INVALID, COSTMAP_4),
    ("autorally_nn_robust", "costmap", dict(array=np.zeros((9, 7, 3))), INVALID, COSTMAP_4),
    ("autorally_nn_robust", "costmap", dict(array=np.zeros((9, 7, 4)), count=251), INVALID, COSTMAP_4),
    ("quadrotor_map", "costmap", dict(array=np.zeros((9, 7, 1))), INVALID, MAP_2 % "costmap"),
    ("quadrotor_map", "costmap", dict(array=np.zeros((9, 7)), dims=(9, 0)), INVALID, MAP_2 % "costmap"),
    # ---- frames of 14 floats
    ("racer_dubins_elevation", "elevation_map_transform", dict(array=np.zeros(14)), INVALID, FRAME % "elevation_map_transform"),
    ("racer_dubins_elevation_suspension", "normals_map_transform", dict(array=np.zeros(14)), INVALID, FRAME % "normals_map_transform"),
    ("quadrotor_map", "costmap_transform", dict(array=np.zeros(14)), INVALID, FRAME % "costmap_transform"),
    # ---- names the model does not have
    ("cartpole", "nope", dict(array=np.zeros(3)), INVALID, "model has no blob named 'nope'"),
    ("autorally_nn", "elevation_map", dict(array=np.zeros((9, 7))), INVALID, "model has no blob named 'elevation_map'"),
    ("racer_dubins_elevation", "normals_map", dict(array=np.zeros((9, 7, 4))), INVALID, "model has no blob named 'normals_map'"),
    ("autorally_nn", "costmap_transform", dict(array=np.zeros(15)), INVALID, "model has no blob named 'costmap_transform'"),
]


def _row_id(row):
    kw = row[2]
    shape = "x".join(str(n) for n in np.shape(kw["array"]))
    return "%s-%s-%s%s%s" % (row[0], row[1], shape, "-count%d" % kw["count"] if "count" in kw else "",
                             "-dims" + "x".join(str(n) for n in kw["dims"]) if "dims" in kw else "")


@pytest.mark.gpu
@pytest.mark.parametrize("row", BLOB_ROWS, ids=_row_id)
def test_set_model_blob_refusal(handle, row):
    key, name, kw, status, text = row
    got = _set_blob(handle(key), name, **kw)
    assert got == (status, text)


H16 = np.zeros(16, np.float32)
STATE_ROWS = [
    ("cartpole", H16, H16, INVALID, "model has no LSTM"),
    ("bicycle_slip_lstm/no-weights", H16, H16, STATE, "set the 'lstm_weights' blob before the initial hidden / cell state"),
    ("bicycle_slip_lstm", np.where(np.arange(16) == 15, np.nan, H16), H16, m.MPPI_ERR_NAN, "non-finite hidden / cell state"),
    ("bicycle_slip_lstm", H16, np.where(np.arange(16) == 0, np.inf, H16), m.MPPI_ERR_NAN, "non-finite hidden / cell state"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("row", STATE_ROWS, ids=["no-lstm", "before-weights", "nan-hidden", "inf-cell"])
def test_set_lstm_initial_state_refusal(handle, row):
    key, hidden, cell, status, text = row
    assert _set_state(handle(key), hidden, cell) == (status, text)


@pytest.mark.gpu
def test_refused_handles_still_run(handle):
    """after every refusal above (whichever ran), the handles that have all they need compute as before"""
    for key in ("autorally_nn", "racer_dubins_elevation_suspension", "autorally_nn_robust", "quadrotor_map"):
        cfg = CONFIGS[key]()
        handle(key).computeControl(cfg["x0"], 1)
    eng = handle("bicycle_slip_lstm")
    assert _set_state(eng, H16 + 0.25, H16 - 0.5)[0] == m.MPPI_OK
    eng.computeControl(CONFIGS["bicycle_slip_lstm"]()["x0"], 1)


# ------------------------------------------------------------------ one accepted blob set per map kind -------------------
ACCEPTED = {
    "elevation_map": (lambda: elevation_cfg(K=K, T=T), make_oracle),
    # "elevation_map", "elevation_map_transform" and "normals_map", no "normals_map_transform": the normals are read in the
    # elevation map's frame (origin (-30, -30), 0.25 m texels; a texture's own default frame is another one)
    "normals_map": (lambda: suspension_cfg(K=K, T=T, maps="both"), make_oracle),
    "costmap-1-channel": (lambda: autorally_cfg(K=K, T=T), make_oracle),
    "costmap-4-channels": (lambda: robust_cfg(K=K, T=T), make_robust_oracle),
    "costmap-texture": (lambda: map_cfg(K=K, T=T), make_map_oracle),
}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(ACCEPTED))
def test_accepted_map_equals_oracle(gpu, plugins, kind):
    build, oracle_of = ACCEPTED[kind]
    cfg = build()
    if kind == "normals_map":
        assert "normals_map" in cfg["blobs"] and "elevation_map_transform" in cfg["blobs"]
        assert "normals_map_transform" not in cfg["blobs"]
    eps = host_noise(1, K, T, len(cfg["std_dev"]), seed=K + T)
    o = oracle_of(cfg)
    eng = make_engine(cfg)
    try:
        if kind == "costmap-texture":  # hover thrust in the mean, as tests/test_quadrotor_map_cost.py flies it
            o.set_nominal_control(nominal_control(T))
            eng.updateImportanceSampler(nominal_control(T))
        o.vanilla_compute_control(cfg["x0"], 1, eps)
        eng.injectNoise(eps)
        eng.computeControl(cfg["x0"], 1)
        dc = int(ulp_diff(eng.getSampledCostSeq(), o.costs()).max())
        du = float(np.abs(eng.getControlSeq() - o.control()).max())
        print("%s: costs %d ulp, u* %.3g" % (kind, dc, du))
        assert np.isfinite(o.costs()).all()
        assert dc == 0, "%s: trajectory costs differ from the oracle by %d ulp" % (kind, dc)
        assert du <= U_TOL, "%s: u* differs from the oracle by %g" % (kind, du)
    finally:
        eng.close()
