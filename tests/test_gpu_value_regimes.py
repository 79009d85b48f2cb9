"""The network and the hash grid in the value regimes of a trained tiny-cuda-nn snapshot (tests/value_regimes.py: tcnn_init, subnormal, amplified, wide, large,
overflow, zero), through the C-ABI on an MI355X.  Every other GPU test draws synth.make_params: a table in U(-0.5, 0.5) with one fp16 subnormal in 10^4 entries, no
activation near 65504, nothing exactly zero.  A snapshot's untouched table entries stay in U(-1e-4, 1e-4), most of them fp16 subnormals, and the hot path meets them
with v_fma_mix_f32 on packed fp16 entries, v_cvt_pk_f16_f32 results in the subnormal range, fp16 A/B fragments of v_mfma_f32_32x32x16_f16, the fp16-accumulating
grid path and the w * 128 fp16 product of the input gradient.

Bars.  Hash-grid features (layer 0) and the SH coefficients: the oracle's bits.  Every matrix layer: the interval of value_regimes.layer_interval, computed in float64
from the DEVICE's own previous layer -- exact sum +- a derived bound of the fp32 summation error, rounded to fp16 on both ends: one fp16 value for 70..99 % of the
units, two adjacent ones for the rest, at any magnitude.  There is no absolute-error clause in this module.  Each regime first asserts, from the oracle on the CPU,
that its inputs are in the regime it is named after.  Frames: tests/test_gpu_parity.py::_compare_frames as it is.

Measured on an MI355X (n = 2051 inputs; every unit of every layer inside its interval in every regime, share 1.000000).  Worst |got - s| / B per layer -- the
ratio is dominated by the fp16 rounding of the stored value (half an fp16 ulp is 2^-12 relative, B about 2^-19 relative), which is why the bar is the interval
rounded to fp16 and not B itself; a layer is one fp16 value for 71..99 % of its units and two adjacent ones for the rest:
               layer1   layer2[:16]   layer3   layer4   outputs
  tcnn_init     128.7       21.7        86.1     40.2     41.7
  subnormal     180.9      134.6       120.1     43.7     33.5
  amplified     104.4       56.3        87.8     41.7     38.2
  wide          126.2       55.7       109.5     50.5     45.5
  large         102.8       54.9       108.0     38.5     40.4
  overflow      102.8       54.3       108.0     38.0     37.9
  zero            0          0           0        0        0      (every layer the oracle's bits)
fp16 accumulators (n = 1027), worst |got - s| / B16, equal to the oracle's own to three digits: tcnn_init 0.63 / 0.22 / 0.23 / 0.28 / 0.22, subnormal 0.78 / 1.28 /
0.30 / 0.31 / 0.20 (1.28: below 2^-14 an fp16 rounding errs by up to 2^-25 absolute, more than the 2^-11 relative B16 counts; the interval's own rounded ends hold it), amplified 0.32 / 0.60 / 0.26 /
0.22 / 0.22, wide 0.51 / 0.54 / 0.40 / 0.22 / 0.22, large 0.34 / 0.57 / 0.27 / 0.26 / 0.25.  Input gradient: wide max rel 3.1e-5 (99.5 % of the vectors identical),
large 7.1e-5 (99.6 %).  Frames (256 x 144, cage edit off / on, records off / on alike): max |dRGBA| tcnn_init 6.6e-6, amplified 9.5e-5, wide 1.1e-4, large 1.5e-4, no
sample count differs; the oracle's frame of `amplified` with a flushed table: max 1.4e-2, mean 5.0e-4, 3.7 % of the sample counts differ.
Nothing on the path flushes or mis-rounds a subnormal on gfx950 ("Value regimes").  The tests print the same figures (`pytest -s`)."""
import copy

import numpy as np
import pytest

import value_regimes as vr
from conftest import GpuRig, Scene
from test_gpu_parity import _compare_frames

pytestmark = pytest.mark.gpu

N_CHAIN = 2048 + 3      # ragged: not a multiple of the 32-sample block, the 64-lane wave or the 128-sample tile
N_CHAIN16 = 1024 + 3
N_GRID = 4096 + 3
N_GRAD = 5000 + 3
_state = {}


def _base(built):
    """One Scene (the conftest scene's occupancy and cage edit) and one GpuRig for the module; a regime swaps params and oracle model in, as
    tests/test_gpu_architectures.py builds its rigs."""
    if "scene" not in _state:
        _state["scene"] = Scene(aabb_scale=1, with_edit=True, lattice_n=6)
        _state["regimes"] = {}
    return _state["scene"]


def _regime_scene(built, name):
    base = _base(built)
    if name not in _state["regimes"]:
        s = copy.copy(base)
        s.params = vr.make_regime(name, base.desc, base.params)
        s.oracle_model = base.orc.Model(base.desc, s.params, base.bitfield)
        _state["regimes"][name] = s
    return _state["regimes"][name]


def _rig(built, name):
    scene = _regime_scene(built, name)
    if "rig" not in _state:
        _state["rig"] = GpuRig(scene)
        _state["rig"].net.set_cell_cache(0)   # (the records are rebuilt on every set_params: on only where they are the subject)
        _state["loaded"] = name
    rig = _state["rig"]
    if _state["loaded"] != name:
        rig.scene = scene
        rig.net.set_params(scene.params)
        _state["loaded"] = name
    rig.scene = scene
    rig.net.set_numerics(0, 0)
    scene.oracle_model.set_numerics(0, 0)
    rig.use_edit(False)
    return rig


@pytest.fixture
def regime_rig(request, built):
    rig = _rig(built, request.param)
    rig.regime = request.param
    yield rig
    rig.net.set_numerics(0, 0)
    rig.scene.oracle_model.set_numerics(0, 0)
    rig.net.set_sparse_cell_cache(None, 0)
    rig.net.set_cell_cache(0)
    rig.use_edit(False)


def _device_chain(rig, c):
    """every dimension of every layer (nrs_network_visualize_activation) and the 16 outputs (nrs_network_inference, interleaved) of the inputs c"""
    torch, n = rig.torch, c.shape[0]
    cin = torch.from_numpy(c).cuda()
    acts = {}
    for layer, width in enumerate(vr.LAYER_WIDTHS):
        out = torch.full((width, n), 7.0, dtype=torch.float32, device="cuda:0")
        for dim in range(width):
            rig.net.visualize_activation(None, layer, dim, cin, out[dim])
        acts[f"layer{layer}"] = np.ascontiguousarray(out.cpu().numpy().T)
    o = torch.full((n, 16), 7.0, dtype=torch.float16, device="cuda:0")
    rig.net.inference_mixed_precision(None, cin, o)
    acts["outputs"] = o.cpu().numpy().astype(np.float32)
    for k, a in acts.items():
        with np.errstate(over="ignore"):
            assert np.array_equal(a.astype(np.float16).astype(np.float32), a, equal_nan=True), k   # fp16 values
    return acts


def _bits(a):
    return np.asarray(a, np.float32).astype(np.float16).view(np.uint16)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _assert_regime(name, scene, c, ref):
    """The precondition of a regime, from the oracle's activations `ref` at the test's own inputs: a regime that drifts out of its regime fails here."""
    table = vr.weights(scene.params)["table"]
    finite = all(np.isfinite(a).all() for a in ref.values())
    biggest = max(float(np.abs(a[np.isfinite(a)]).max()) for a in ref.values())
    if name in ("tcnn_init", "subnormal", "amplified"):
        assert vr.is_subnormal(table[:1 << 22]).mean() > 0.5 and vr.is_subnormal(ref["layer0"]).mean() >= 0.5 and finite
        if name == "subnormal":   # hidden units (the half ReLU leaves) and the density network's outputs (but for the constant channel's) are subnormal too
            assert vr.is_subnormal(ref["layer1"]).mean() > 0.3 and vr.is_subnormal(ref["layer2"][:, 1:16]).mean() > 0.9
        if name == "amplified":
            assert ref["layer1"][:, 1:].std(axis=0).max() > 0.05 and ref["layer1"].max() > 0.25   # the features, not a constant, decide O(1) hidden values
    elif name == "wide":
        seen = set(_bits(ref["layer0"]).ravel().tolist())
        assert {0x0000, 0x0001, 0x8001, 0x0400, 0x03ff, 0x7bff} <= seen, "the planted values are not read back at the planted positions"
        assert finite and vr.is_subnormal(ref["layer0"]).mean() > 0.01 and ref["layer0"].max() == 65504
    elif name == "large":
        assert finite and 1e3 <= float(ref["layer1"].max()) and biggest <= 32752, biggest     # below 65504 / 2
        assert (ref["layer1"] > 1e3).mean() > 0.05 and ref["layer3"].max() > 100
    elif name == "overflow":
        cls1, cls2 = vr.value_class(ref["layer1"]), vr.value_class(ref["layer2"])
        assert (cls1 == 1).sum() >= 1 and (cls1 == 1).mean() < 0.01 and (cls2 == 1).sum() >= 1 and (cls2 == 2).sum() >= 1   # a few units, +inf and -inf downstream
    elif name == "zero":
        assert finite and not ref["layer3"].any() and not ref["layer0"][:, 1:].any()


@pytest.mark.parametrize("regime_rig", vr.REGIMES, indirect=True)
def test_chain_layer_by_layer(regime_rig):
    """Section by section of the chain, default numerics: layer 0 and the SH half of layer 2 are the oracle's bits, every matrix layer lies in the interval its own
    (device) inputs give, output 3 is layer 2's unit 0.  `inference` in both layouts, a padded planes buffer and `density` are the same numbers."""
    rig, torch, name = regime_rig, regime_rig.torch, regime_rig.regime
    scene = rig.scene
    c = vr.regime_coords(name, scene.desc, N_CHAIN, 5)
    ref = vr.oracle_activations(scene.oracle_model, c)
    _assert_regime(name, scene, c, ref)
    # ---- the GPU
    acts = _device_chain(rig, c)
    assert np.array_equal(_bits(acts["layer0"]), scene.oracle_model.hashgrid_encode(c)) and _same_bits(acts["layer0"], ref["layer0"])
    assert _same_bits(acts["layer2"][:, 16:], ref["layer2"][:, 16:])
    report, failures = vr.check_chain(acts, scene.params)
    for layer, r in report.items():
        print(f"[{name}] {layer}: inside {r['inside']:.6f}, worst |got - s| / B {r['worst_over_B']:.1f}, one-value intervals {r['single_value']:.3f}")
    assert not failures, failures
    # the other entry points give the same numbers
    cin = torch.from_numpy(c).cuda()
    n = c.shape[0]
    planes = torch.full((16, n), 7.0, dtype=torch.float16, device="cuda:0")
    rig.net.inference_mixed_precision(None, cin, planes)
    assert _same_bits(planes.cpu().numpy().T, acts["outputs"])
    padded = torch.full((16, n + 61), 7.0, dtype=torch.float16, device="cuda:0")
    rig.net.inference_mixed_precision(None, cin, padded)
    padded = padded.cpu().numpy()
    assert (padded[:, n:] == 7.0).all() and _same_bits(padded[:, :n].T, acts["outputs"])
    dens = torch.full((16, n), 7.0, dtype=torch.float16, device="cuda:0")
    rig.net.density(None, torch.from_numpy(np.ascontiguousarray(c[:, :3])).cuda(), dens)
    dens = dens.cpu().numpy().T.astype(np.float64)
    lo, hi, _, _ = vr.layer_interval(acts["layer1"], vr.weights(scene.params)["dw2"], False)
    assert vr.inside(dens, lo, hi).all(), "density() leaves the interval of its own hidden layer"
    # ---- against the oracle where the regime says so
    if name == "overflow":
        for k in acts:
            assert np.array_equal(vr.value_class(acts[k]), vr.value_class(ref[k])), f"{k}: finite / +inf / -inf / NaN differ from the oracle's"
    if name == "zero":
        for k in acts:
            assert _same_bits(acts[k], ref[k]), k
        assert np.array_equal(_bits(dens), scene.oracle_model.density(c[:, :3], 1))


@pytest.mark.parametrize("regime_rig", vr.REGIMES, indirect=True)
def test_hashgrid_every_route(regime_rig):
    """hashgrid_encode is the oracle's bits with both grid roundings, without cell records, with the dense ones and with the sparse ones: the records repack the
    same fp16 bits, a subnormal survives the repack."""
    rig, torch, name = regime_rig, regime_rig.torch, regime_rig.regime
    scene = rig.scene
    c = vr.regime_coords(name, scene.desc, N_GRID, 11)
    cin = torch.from_numpy(c).cuda()
    for grid_acc in (0, 1):
        rig.net.set_numerics(grid_acc, 0)
        scene.oracle_model.set_numerics(grid_acc, 0)
        ref = scene.oracle_model.hashgrid_encode(c)
        if name in ("tcnn_init", "subnormal", "amplified"):
            assert vr.is_subnormal(ref.view(np.float16)).mean() >= 0.5
        if name == "wide":
            assert {0x0001, 0x8001, 0x0400, 0x03ff, 0x7bff} <= set(ref.ravel().tolist())
        for route in ("none", "dense", "sparse"):
            rig.net.set_sparse_cell_cache(None, 0)
            rig.net.set_cell_cache(1 << 30 if route == "dense" else 0)
            if route == "dense":
                assert rig.net.cell_cache()[1] >= 2
            if route == "sparse":
                rig.net.set_sparse_cell_cache(scene.bitfield, 2 << 30)
                assert rig.net.sparse_cell_cache()[2] >= 2 and rig.net.sparse_cell_cache()[1] == 0
            out = torch.zeros((c.shape[0], 32), dtype=torch.float16, device="cuda:0")
            rig.net.hashgrid_encode(None, cin, out)
            got = out.cpu().numpy().view(np.uint16)
            assert np.array_equal(got, ref), f"[{name} grid_acc {grid_acc} records {route}] {(got != ref).sum()} of {got.size} features differ"


@pytest.mark.parametrize("regime_rig", ["tcnn_init", "subnormal", "amplified", "wide", "large"], indirect=True)
def test_fp16_accumulators(regime_rig):
    """set_numerics(1, 1): the device's chain and the oracle's model of it both lie in the interval with B16 (one fp16 rounding of the running sum per 16-wide
    block and one of the output), each from its own previous layer.  (`overflow` is left out: a running sum rounded to fp16 may leave fp16 where the whole sum
    does not, which B16 does not model.)"""
    rig, name = regime_rig, regime_rig.regime
    scene = rig.scene
    c = vr.regime_coords(name, scene.desc, N_CHAIN16, 6)
    rig.net.set_numerics(1, 1)
    scene.oracle_model.set_numerics(1, 1)
    ref = vr.oracle_activations(scene.oracle_model, c)
    if name in ("tcnn_init", "subnormal", "amplified"):
        assert vr.is_subnormal(ref["layer0"]).mean() >= 0.5
    if name == "subnormal":
        assert vr.is_subnormal(ref["layer1"]).mean() > 0.3 and vr.is_subnormal(ref["layer2"][:, 1:16]).mean() > 0.9
    if name == "large":
        assert 1e3 <= float(ref["layer1"].max()) and max(float(np.abs(a).max()) for a in ref.values()) <= 32752
    ref_report, ref_failures = vr.check_chain(ref, scene.params, acc16=True)
    assert not ref_failures, ("the oracle's own fp16-accumulator model leaves B16", ref_failures)
    acts = _device_chain(rig, c)
    assert _same_bits(acts["layer0"], ref["layer0"]) and _same_bits(acts["layer2"][:, 16:], ref["layer2"][:, 16:])
    report, failures = vr.check_chain(acts, scene.params, acc16=True)
    for layer, r in report.items():
        print(f"[{name} fp16 accumulators] {layer}: inside {r['inside']:.6f}, worst |got - s| / B16 {r['worst_over_B']:.3f} (oracle {ref_report[layer]['worst_over_B']:.3f})")
    assert not failures, failures


@pytest.mark.parametrize("regime_rig", ["amplified", "wide", "large"], indirect=True)
def test_input_gradient(regime_rig):
    """nrs_network_input_gradient with the bars of tests/test_gpu_introspection.py::test_input_gradient_operator: large weights, subnormal dL/dfeature factors and the
    fp16 product w * 128."""
    rig, torch, name = regime_rig, regime_rig.torch, regime_rig.regime
    c = vr.regime_coords(name, rig.scene.desc, N_GRAD, 9)
    ref = rig.scene.oracle_model.density_input_gradient(c).astype(np.float64)
    # (`amplified`: W1 ~ 1000 times the loss scale 128 takes a dL/dfeature factor of one sample in 5003 past fp16: that row is +-inf in the oracle, and must be here)
    finite = np.isfinite(ref).all(axis=1)
    norm = np.linalg.norm(ref[finite], axis=1)
    assert finite.mean() >= 0.999 and (norm > 0).mean() >= 0.9, "the regime has no gradients to compare"
    out = torch.zeros((c.shape[0], 3), dtype=torch.float32, device="cuda:0")
    rig.net.input_gradient(None, torch.from_numpy(c).cuda(), out)
    got = out.cpu().numpy().astype(np.float64)
    assert np.array_equal(vr.value_class(got), vr.value_class(ref)), "finite / +inf / -inf / NaN differ from the oracle's"
    got, ref = got[finite], ref[finite]
    scale = np.maximum(norm, 1e-3 * norm.max())
    rel = np.linalg.norm(got - ref, axis=1) / scale
    print(f"[{name} input gradient] non-zero {(norm > 0).mean():.3f}, median rel {np.median(rel):.2e}, 99th percentile {np.quantile(rel, 0.99):.2e}, max {rel.max():.2e}, identical {np.all(got == ref, axis=1).mean():.3f}")
    assert np.quantile(rel, 0.99) <= 1e-3 and rel.max() <= 2e-2 and np.all(got == ref, axis=1).mean() >= 0.95, (np.quantile(rel, 0.99), rel.max())


def _flush_is_visible(scene, p, edits, ref):
    """The oracle's frame of the table with its subnormals flushed misses _compare_frames' bars by a wide margin: a frame test in this regime sees a flush."""
    flushed = scene.orc.Model(scene.desc, vr.flush_subnormals(scene.params), scene.bitfield)
    f, d, s, _ = flushed.render(p, edits)
    err = np.abs(f - ref[0])
    steps_differ = (s != ref[2]).mean()
    print(f"[flushed table, oracle against oracle] max {err.max():.3e}, mean {err.mean():.3e}, steps differ {steps_differ:.4f}")
    assert err.max() > 2 * 6e-3 and err.mean() > 2 * 2e-4 and steps_differ > 10 * 0.002
    with pytest.raises(AssertionError):
        _compare_frames(f, d, s, ref[0], ref[1], ref[2])


@pytest.mark.parametrize("edit", [False, True])
@pytest.mark.parametrize("regime_rig", ["tcnn_init", "amplified", "wide", "large"], indirect=True)
def test_frames(regime_rig, edit):
    """The fused render kernel has its own copy of the path (LDS slabs, rounding through the matrix core): one frame per regime, cage edit off and on, cell records
    off and on, against the oracle with the frame bars as they are."""
    rig, name = regime_rig, regime_rig.regime
    scene = rig.scene
    rig.use_edit(edit)
    p = scene.params_for(256, 144, 60.0)
    edits = [scene.oracle_edit] if edit else []
    ref = scene.oracle_model.render(p, edits)
    assert ref[3].n_hit > 1000 and not np.isnan(ref[0]).any()
    if name == "amplified" and not edit:
        _flush_is_visible(scene, p, edits, ref)
    for cache in (0, 10 << 30):
        rig.net.set_cell_cache(cache)
        assert (rig.net.cell_cache()[1] > 0) == (cache > 0)
        frame, depth, steps, stats = rig.render(p)
        assert stats.n_rays_alive == ref[3].n_alive0
        d = np.abs(frame - ref[0])
        print(f"[{name} edit {edit} records {cache > 0}] max {d.max():.3e}, mean {d.mean():.3e}, steps equal {(steps == ref[2]).mean():.5f}")
        _compare_frames(frame, depth, steps, ref[0], ref[1], ref[2])


@pytest.mark.parametrize("regime_rig", ["overflow"], indirect=True)
def test_overflow_frame_has_no_nan(regime_rig):
    """Where a hidden unit leaves fp16 the frame stays free of NaN wherever the oracle's is."""
    rig = regime_rig
    p = rig.scene.params_for(256, 144, 60.0)
    ref = rig.scene.oracle_model.render(p, [])
    frame, depth, _, _ = rig.render(p)
    assert ref[3].n_hit > 1000
    assert not (np.isnan(frame) & ~np.isnan(ref[0])).any() and not (np.isnan(depth) & ~np.isnan(ref[1])).any()


@pytest.mark.parametrize("regime_rig", ["amplified"], indirect=True)
def test_encoding_vis_of_a_hidden_unit(regime_rig):
    """NRS_RENDER_ENCODING_VIS of a density hidden unit in `amplified` (the bar of tests/test_gpu_introspection.py::test_render_mode_encoding_vis)."""
    rig = regime_rig
    scene = rig.scene
    rig.use_edit(True)
    p = scene.params_for(192, 108, 60.0)
    p.render_mode, p.visualized_layer, p.visualized_dimension = 11, 1, 20
    ref_frame, ref_depth, ref_steps, ref_stats = scene.oracle_model.render(p, [scene.oracle_edit])
    frame, depth, steps, stats = rig.render(p)
    assert ref_stats.n_hit > 500 and stats.n_rays_alive == ref_stats.n_alive0
    assert np.abs(ref_frame[..., :2]).max() > 0.05   # the unit is alive in the picture
    scale = max(1.0, float(np.abs(ref_frame[..., :3]).max()))
    d = np.abs(frame - ref_frame)
    ds = np.abs(steps.astype(np.int64) - ref_steps.astype(np.int64))
    print(f"[amplified encoding vis 1/20] max {d.max():.3e} (scale {scale:.2f}), mean {d.mean():.3e}, steps equal {(ds == 0).mean():.5f}")
    assert d.max() < 6e-3 * scale and d.mean() < 2e-4 * scale
    assert ds.max() <= 1 and (ds == 0).mean() >= 0.998
    assert (frame[..., 2] == 0).all()
