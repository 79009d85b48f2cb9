"""CPU-only tests of the light-direction entry points (n_extra_dims = 3): parameter counts, refusals, the snapshot reader with NRS_SNAPSHOT_ALLOW_LIGHT_DIRS."""
import ctypes as C
import os

import numpy as np
import pytest

from nerfshop_amd import _abi, formats, synth

NEW = ("nrs_model_create_ex", "nrs_model_n_params_ex", "nrs_model_n_extra_dims", "nrs_model_set_light_dir", "nrs_network_inference_strided",
       "nrs_snapshot_open_ex", "nrs_snapshot_n_extra_dims")


def test_exports_and_abi_version(built):
    lib = _abi.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nrs.h")).read()
    for name in NEW:
        assert name in _abi.EXPORTS and hasattr(lib, name) and f"{name}(" in header
    assert lib.nrs_abi_version() == 3   # appended exports: no layout changed


@pytest.mark.parametrize("layers", [1, 2, 3])
def test_n_params_ex(built, layers):
    lib = _abi.load()
    desc = synth.model_desc(1, rgb_hidden_layers=layers)
    plain = lib.nrs_model_n_params(C.byref(desc))
    assert plain > 0 and lib.nrs_model_n_params_ex(C.byref(desc), 0) == plain
    assert lib.nrs_model_n_params_ex(C.byref(desc), 3) == plain + 1024
    assert synth.make_light_params(desc).size == plain + 1024


def test_n_params_ex_refusals(built):
    lib = _abi.load()
    base = synth.model_desc(1)
    for n_extra in (1, 2, 4, 16):
        assert lib.nrs_model_n_params_ex(C.byref(base), n_extra) == 0
    assert lib.nrs_model_n_params_ex(C.byref(synth.model_desc(1, no_dir=True)), 3) == 0          # NerfNetworkNoDir
    assert lib.nrs_model_n_params_ex(C.byref(synth.model_desc(1, rgb_hidden_layers=0)), 3) == 0   # the 0-layer CutlassMLP rgb network
    assert lib.nrs_model_n_params_ex(None, 3) == 0
    # no device is needed to be turned away: the argument checks come first
    h = C.c_void_p()
    assert lib.nrs_model_create_ex(None, C.byref(base), 3, C.byref(h)) == -1
    assert lib.nrs_model_set_light_dir(None, None) == -1 and lib.nrs_model_n_extra_dims(None) == 0


def test_add_light_columns_layout(built):
    """the first rgb matrix becomes [64 x 48] row-major; everything else of the blob keeps its order"""
    desc = synth.model_desc(1)
    plain = synth.make_params(desc)
    cols = np.arange(64 * 16, dtype=np.float32).reshape(64, 16) / 1024.0
    light = synth.add_light_columns(desc, plain, cols)
    o = 64 * 32 + 16 * 64
    w1 = light[o: o + 64 * 48].reshape(64, 48)
    assert np.array_equal(light[:o], plain[:o]) and np.array_equal(light[o + 64 * 48:], plain[o + 64 * 32:])
    assert np.array_equal(w1[:, :32], plain[o: o + 64 * 32].reshape(64, 32))
    assert np.array_equal(w1[:, 32:].view(np.float16).astype(np.float32), cols)


@pytest.mark.parametrize("name,exported", [("light.msgpack", False), ("light.ingp", True)])
def test_snapshot_with_light_dirs(built, tmp_path, name, exported):
    """the harness-written file comes back bit for bit with the flag and reports 3; without it -- and through nrs_snapshot_open -- it is still refused.  The saved file
    carries has_light_dirs, the exported one is recognised by the size of its blob alone."""
    lib = _abi.load()
    desc = synth.model_desc(1)
    params = synth.make_light_params(desc)
    grid = synth.density_grid(1)
    path = tmp_path / name
    formats.save_snapshot(path, desc, 1, params, grid, exported=exported, has_light_dirs=True)
    s = formats.load_snapshot(path, allow_light_dirs=True)
    assert s.n_extra_dims == 3 and np.array_equal(s.params, params)
    assert s.desc.rgb_hidden_layers == 2 and s.desc.sh_degree == 4
    assert lib.nrs_model_n_params_ex(C.byref(s.desc), s.n_extra_dims) == params.size
    with pytest.raises(_abi.NrsError) as ei:
        formats.load_snapshot(path)
    assert "nrs error -2" in str(ei.value) and ("light directions" in str(ei.value))
    h = C.c_void_p()
    assert lib.nrs_snapshot_open_ex(str(path).encode(), 0, C.byref(h)) == -2
    assert lib.nrs_snapshot_open_ex(str(path).encode(), 2, C.byref(h)) == -1   # unknown flag
    # a plain snapshot opened with the flag is a plain snapshot
    plain = synth.make_params(desc)
    formats.save_snapshot(tmp_path / ("plain_" + name), desc, 1, plain, grid, exported=exported)
    sp = formats.load_snapshot(tmp_path / ("plain_" + name), allow_light_dirs=True)
    assert sp.n_extra_dims == 0 and np.array_equal(sp.params, plain)


def test_snapshot_light_dirs_outside_the_family(built, tmp_path):
    """light directions with NerfNetworkNoDir or the 0-layer rgb network: NRS_ERR_UNSUPPORTED, named"""
    grid = synth.density_grid(1)
    for kw, word in (({"no_dir": True}, "NerfNetworkNoDir"), ({"rgb_hidden_layers": 0}, "0-layer")):
        desc = synth.model_desc(1, **kw)
        path = tmp_path / "odd.msgpack"
        formats.save_snapshot(path, desc, 1, synth.make_params(desc), grid, exported=False, has_light_dirs=True)
        with pytest.raises(_abi.NrsError) as ei:
            formats.load_snapshot(path, allow_light_dirs=True)
        assert "nrs error -2" in str(ei.value) and word in str(ei.value)
