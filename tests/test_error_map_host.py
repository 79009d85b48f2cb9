"""The training error map without a GPU: the surface, nrs_error_map_cdfs_host bit for bit against the twin of tests/error_map_ref.py, the properties every CDF must
have, nrs_error_map_resolution against the reference's formula and its clamps, the twin's own sampling, and the refusals that need no device.

Every test that touches the library fails without the feature (the symbols are missing); test_twin_sampling_goes_where_the_error_is pins the twin the GPU tests
compare with.  The bar on pmf * width, 0.009, is below MIN_PDF = 0.01 by what float32 loses in a difference of two CDF entries near 1: an entry carries an error of
about 2^-24, the smallest pmf at width 1024 is 0.01 / 1024 = 9.8e-6, so pmf * width is off by up to 2 * 2^-24 * 1024 = 1.2e-4 -- 0.0099 at worst; the twin's own worst
on these inputs, checked here in float32 and printed, is 0.00995 at width 1024."""
import ctypes as C
import os

import numpy as np
import pytest

import error_map_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
SHAPES = [(1, 2, 2), (3, 3, 5), (7, 29, 29), (2, 2, 1024), (2, 1024, 2)]
f32 = np.float32


def maps(shape):
    """the inputs of the CDF tests for one shape: name -> float32 map"""
    n, res_y, res_x = shape
    rng = np.random.default_rng(n * 1000003 + res_y * 1009 + res_x)
    out = {"zero": np.zeros(shape, f32)}
    for name, x in (("spike_first", 0), ("spike_last", res_x - 1)):
        m = (rng.random(shape) * 1e-3).astype(f32)
        m[n - 1, res_y // 2, x] = 1e6
        out[name] = m
    out["heavy_tail"] = (rng.pareto(0.7, shape) * 1e-4).astype(f32)   # a few cells hold nearly everything
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all()


def check_cdf(cdf, name):
    """non-decreasing along the last axis, last entry within one float32 step of 1, every pmf * width >= 0.009; returns the worst pmf * width"""
    width = cdf.shape[-1]
    pmf = np.diff(np.concatenate([np.zeros(cdf.shape[:-1] + (1,), f32), cdf], -1), axis=-1)
    assert (pmf >= 0).all(), name + " decreases"
    last = cdf[..., -1].astype(np.float64)
    assert ((last >= 1.0 - 2.0 ** -24) & (last <= 1.0 + 2.0 ** -23)).all(), name + " does not end within one float32 step of 1"
    worst = float((pmf * f32(width)).min())
    assert worst >= 0.009, (name, worst)
    return worst


def test_surface_exists(built):
    from nerfshop_amd import _abi, runtime, trainer
    lib = _abi.load()
    header = open(os.path.join(ROOT, "include", "nrs.h")).read()
    for name in ("nrs_dataset_error_map_reset", "nrs_error_map_resolution", "nrs_dataset_error_map_set", "nrs_dataset_error_map_get", "nrs_dataset_error_map_accumulate",
                 "nrs_dataset_error_map_build_cdfs", "nrs_error_map_cdfs_host", "nrs_dataset_rays_ex"):
        assert name in _abi.EXPORTS and hasattr(lib, name) and f"{name}(" in header, name
    assert lib.nrs_abi_version() == 3, "new surface, detected by symbol: no existing layout changes"
    assert C.sizeof(_abi.DatasetRaysParams) == 32, "nrs_dataset_rays keeps its struct"
    assert C.sizeof(_abi.DatasetRaysExParams) == 40 == _abi.DatasetRaysExParams().struct_size
    assert [f[0] for f in _abi.DatasetRaysExParams._fields_][:6] == [f[0] for f in _abi.DatasetRaysParams._fields_], "the present fields come first"
    assert (_abi.ERROR_MAP_FLOAT, _abi.ERROR_MAP_CDF_X_COND_Y, _abi.ERROR_MAP_CDF_Y, _abi.ERROR_MAP_CDF_IMG, _abi.ERROR_MAP_PMF_IMG, _abi.ERROR_MAP_CELLS) == (0, 1, 2, 3, 4, 5)
    for method in ("error_map_reset", "error_map_set", "error_map_get", "error_map_accumulate", "error_map_build_cdfs", "error_map_resolution", "rays"):
        assert callable(getattr(runtime.Dataset, method))
    assert "by_error" in runtime.Dataset.rays.__doc__
    s = trainer.ErrorMapSchedule()
    assert (s.steps_between, s.growth, s.sample_images, s.sample_pixels) == (128, 1.5, False, False)
    import inspect
    for fn in (trainer.Trainer.step_dataset, trainer.Trainer.fit):
        assert inspect.signature(fn).parameters["error_map"].default is None
    compat = open(os.path.join(ROOT, "include", "nrs_compat.hpp")).read()
    for name in ("error_map_reset", "error_map_set", "error_map_get", "error_map_accumulate", "error_map_build_cdfs", "nrs_dataset_rays_ex"):
        assert name in compat, name


@pytest.mark.parametrize("shape", SHAPES)
def test_cdfs_host_against_the_twin(built, shape):
    from nerfshop_amd import runtime
    for name, m in maps(shape).items():
        got = runtime.error_map_cdfs_host(m)
        want = ref.cdfs(m)
        for g, w, what in zip(got, want, ("cdf_x_cond_y", "cdf_y", "cdf_img", "pmf_img")):
            assert same_bits(g, w), (shape, name, what)
        worst = [check_cdf(c, f"{shape} {name} {what}") for c, what in zip(got[:3], ("cdf_x_cond_y", "cdf_y", "cdf_img"))]
        pmf_img = got[3]
        assert (pmf_img * f32(shape[0]) >= f32(0.09)).all() and abs(float(pmf_img.astype(np.float64).sum()) - 1.0) < 1e-5, "MIN_PMF = 0.1 over the images"
        print(f"{shape} {name}: worst pmf * width: cdf_x_cond_y {worst[0]:.5f} cdf_y {worst[1]:.5f} cdf_img {worst[2]:.5f}")


def test_cdfs_follow_the_map(built):
    """what the CDFs are for: the spike's row, column and image get nearly all of the non-uniform mass"""
    from nerfshop_amd import runtime
    shape = (7, 29, 29)
    m = maps(shape)["spike_last"]
    cx, cy, ci, pi = runtime.error_map_cdfs_host(m)
    row = 29 // 2
    assert cx[6, row, 28] - cx[6, row, 27] > 0.98 and cy[6, row] - cy[6, row - 1] > 0.98 and pi[6] > 0.9 and ci[6] - ci[5] > 0.9
    assert same_bits(ci[-1:], np.ones(1, f32)) or abs(float(ci[-1]) - 1.0) <= 2.0 ** -23


def test_resolution_formula_and_clamps(built):
    from nerfshop_amd import _abi, runtime

    def formula(steps, rays, n_images):
        per_image = ((steps * rays) & 0xffffffff) // n_images
        return int(np.sqrt(np.sqrt(f32(per_image), dtype=f32), dtype=f32) * f32(3.5))
    for steps, rays, n_images, res in ((128, 4096, 100, 800), (128, 4096, 8, 800), (4, 1024, 8, 32), (128, 1 << 18, 3, 4000), (1, 1, 1000, 64), (192, 4096, 1025, 48),
                                       (1 << 20, 1 << 13, 2, 512)):
        want = min(max(formula(steps, rays, n_images), 2), min(res, _abi.ERROR_MAP_MAX_RESOLUTION))
        assert runtime.error_map_resolution(steps, rays, n_images, res) == want, (steps, rays, n_images, res)
    assert runtime.error_map_resolution(128, 4096, 100, 800) == formula(128, 4096, 100) == 29, "the reference's defaults on 100 images"
    assert runtime.error_map_resolution(4, 1024, 8, 32) == 16
    assert runtime.error_map_resolution(1, 1, 1000, 64) == 2, "clamped from below"
    # (the formula itself stays below 2^8 * 3.5 = 896 -- its argument has 32 bits -- so from above only the image resolution ever clamps)
    assert runtime.error_map_resolution(128, 1 << 18, 3, 4000) == 202 and runtime.error_map_resolution(128, 4096, 8, 20) == 20, "clamped from above"
    assert runtime.error_map_resolution(0xffffffff, 1, 1, 4000) == formula(0xffffffff, 1, 1) == 896 and runtime.error_map_resolution(0xffffffff, 1, 1, 300) == 300
    assert runtime.error_map_resolution(1 << 20, 1 << 13, 2, 512) == 2, "the product wraps in 32 bits, as the reference's"
    assert runtime.error_map_resolution(128, 4096, 0, 800) == 0 and runtime.error_map_resolution(128, 4096, 8, 1) == 0, "no map is possible"


def test_quantise_rule():
    """the twin's deposit rule on the cases of the GPU test: zero, NaN, negative, 1e9, sub-2^-32, and exactness of the scaling"""
    q = ref.quantise(np.array([0.0, np.nan, -1.0, 1e9, 2.0 ** -33, 2.0 ** -32, 1.0, 0.3, np.inf, 1024.0, 1e-45], f32))
    assert q == [0, 0, 0, 1 << 42, 0, 1, 1 << 32, int(f32(0.3) * f32(2.0 ** 32)), 1 << 42, 1 << 42, 0]
    assert int(np.float64(f32(0.3)) * 2.0 ** 32) == q[7], "the float32 product is exact"
    assert (1 << 21) * (1 << 42) < 1 << 64, "2^21 deposits of the clamp value fit"
    assert same_bits(ref.cells_to_float([0, 1, 1 << 32, (1 << 42) + 1]), np.array([0, 2.0 ** -32, 1.0, 1024.0], f32))


def test_twin_sampling_goes_where_the_error_is(built):
    """All the error in one cell: half of the rays are uniform, the other half follows CDFs that give the cell (1 - MIN_PDF)^2 of their mass plus its share of the
    uniform floor -- 0.5 * 0.99^2 = 0.49 of all rays expected in the cell's pixels.  Seed 1337 (dataset_ref.draws), 4096 rays, one image."""
    n_rays, W, H, res = 4096, 64, 48, 8
    m = np.zeros((1, res, res), f32)
    m[0, 5, 2] = 1.0
    cx, cy, ci, _ = ref.cdfs(m)
    for snap in (True, False):
        s = ref.sample(1337, n_rays, 0, 1, W, H, snap, (cx, cy, ci), False, True)
        px, py = s["pixel"] % W, s["pixel"] // W
        inside = (px // (W // res) == 2) & (py // (H // res) == 5)
        share = float(inside.mean())
        print(f"snap {snap}: {share:.4f} of {n_rays} rays in the cell's pixels; {float(s['cdf_half'].mean()):.4f} drawn from the CDFs")
        assert share >= 0.45
        assert (s["pdf"][~s["cdf_half"]] == 1).all() and (s["pdf"][s["cdf_half"] & inside] > 50).all(), "the CDF half's density alone: 0.99^2 * 64 in the cell"
        assert (s["xy"] >= 0).all() and (s["xy"] <= 1).all()


def test_refusals_without_a_device(built):
    from nerfshop_amd import _abi
    lib = _abi.load()
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    assert lib.nrs_dataset_error_map_reset(None, 4, 4, None) == INVALID
    assert lib.nrs_dataset_error_map_set(None, 4, 4, p) == INVALID
    assert lib.nrs_dataset_error_map_get(None, 0, p, None) == INVALID
    assert lib.nrs_dataset_error_map_accumulate(None, None, 1, p, p, p, p, p, None, None) == INVALID
    assert lib.nrs_dataset_error_map_build_cdfs(None, None) == INVALID
    assert lib.nrs_dataset_rays_ex(None, None, C.byref(_abi.DatasetRaysExParams()), 1, p, p, p, p, p, p, p) == INVALID
    assert b"NULL" in lib.nrs_last_error()
    for args in ((1, 2, 2, None, p, p, p, p), (1, 2, 2, p, None, p, p, p), (1, 2, 2, p, p, p, p, None), (0, 2, 2, p, p, p, p, p), (1, 0, 2, p, p, p, p, p), (1, 2, 0, p, p, p, p, p)):
        assert lib.nrs_error_map_cdfs_host(*args) == INVALID, args
    from nerfshop_amd import trainer
    with pytest.raises(_abi.NrsError):
        trainer.ErrorMapSchedule(steps_between=0)
    with pytest.raises(_abi.NrsError):
        trainer.ErrorMapSchedule(growth=0.5)
