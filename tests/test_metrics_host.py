"""Image metrics without a GPU: the surface, the refusals that need no device, the reflect blur of tests/metrics_ref.py against scipy, the CPU twin
nrs_image_metrics_host against the float64 restatement, identical images, run.py's totals, and the twin under the address and undefined-behaviour sanitizers as a
stand-alone program (tests/metrics_host_check.cpp).  Every test that touches the library fails without the feature (the symbols are missing).

THE BARS.  Mean ssim within 2e-5 absolute, mse within 1e-5 relative, the per-pixel ssim map within 1e-3.  They come from a measurement of the reference's own float32
data flow (numpy float32 through the same formulas) against the float64 restatement on these shapes: at most 3.1e-6 in mean ssim and 3.3e-4 per pixel, with a
x3 - x6 margin for powf and contraction differences.  Measured for the twin on the inputs of this file (printed by the test): mean ssim at most 1.6e-6, mse at most
1.3e-6 relative (a 1 x 1 image: one pixel's powf), per pixel at most 1.9e-4 -- each below a third of its bar (profiles/eval_metrics.md).

THE SUMS AGAINST THE MAPS.  sum_ssim equals the sum of round(ssim_map * 2^32) exactly: the map holds the very float32 that was rounded.  The squared-error map holds
the float32 mean of the three channels, m = fl(fl(fl(e_r + e_g) + e_b) / 3), from which the three terms cannot be recovered; with u = 2^-24 and e_c <= 1,
|3 m - (e_r + e_g + e_b)| <= 3 u * 3 = 2304 * 2^-32, and the four roundings to integers add at most 2: |sum_sq_err - sum round(3 m * 2^32)| <= 2306 n."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import metrics_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
NAMES = ("nrs_image_metrics", "nrs_dataset_image_metrics", "nrs_image_metrics_host", "nrs_image_metrics_summary_host")
SHAPES = [(1, 1), (2, 3), (5, 7), (37, 53), (64, 96)]   # (height, width)
f32 = np.float32


def test_surface_exists(built):
    from nerfshop_amd import _abi, runtime, trainer
    from nerfshop_amd.runtime import metrics
    lib = _abi.load()
    header = open(os.path.join(ROOT, "include", "nrs.h")).read()
    for name in NAMES:
        assert name in _abi.EXPORTS and hasattr(lib, name) and f"{name}(" in header, name
    assert "#define NRS_ABI_VERSION 3 " in header and lib.nrs_abi_version() == 3, "new surface, detected by symbol: no existing layout changes"
    assert C.sizeof(_abi.ImageMetricsResult) == 32 == metrics.RECORD_BYTES == np.dtype(_abi.METRICS_RECORD_DTYPE).itemsize
    assert C.sizeof(_abi.ImageMetricsParams) == 28 == _abi.ImageMetricsParams().struct_size
    assert f"#define NRS_IMAGE_METRICS_MAX_DIM {_abi.IMAGE_METRICS_MAX_DIM}u" in header
    assert "(-1, -1, -1, -1) gets NO special case" in header, "the header says what happens to a masked pixel"
    for fn in (runtime.image_metrics, runtime.image_metrics_host, runtime.metrics_summary, runtime.Dataset.image_metrics, runtime.Testbed.evaluate, trainer.Trainer.evaluate):
        assert callable(fn)
    assert "tonemap" in runtime.Testbed.evaluate.__doc__
    compat = open(os.path.join(ROOT, "include", "nrs_compat.hpp")).read()
    for name in ("image_metrics", "nrs_dataset_image_metrics", "nrs_image_metrics_summary_host"):
        assert name in compat, name
    assert "nrs_metrics.hip" in open(os.path.join(ROOT, "nerfshop_amd", "csrc", "Makefile")).read()


def test_refusals_without_a_device(built):
    from nerfshop_amd import _abi
    lib = _abi.load()
    img = np.zeros((2, 3, 4), f32)
    rf = np.zeros((2, 3, 4), f32)
    res = _abi.ImageMetricsResult()
    P = lambda a: a.ctypes.data   # noqa: E731

    def host(width=3, height=2, image=P(img), reference=P(rf), params=None, result=C.addressof(res), **fields):
        p = _abi.ImageMetricsParams()
        p.reference_format = _abi.IMAGE_RGBA32F_LINEAR
        for k, v in fields.items():
            if k == "background_color":
                p.background_color[:] = v
            else:
                setattr(p, k, v)
        return lib.nrs_image_metrics_host(width, height, image, reference, C.byref(p) if params is None else params, result, None, None)
    assert host() == 0
    for kw in (dict(image=None), dict(reference=None), dict(params=C.POINTER(_abi.ImageMetricsParams)()), dict(result=None)):
        assert host(**kw) == INVALID and b"NULL" in lib.nrs_last_error(), kw
    for kw, word in ((dict(width=0), b"is 0"), (dict(height=0), b"is 0"), (dict(width=8193), b"8192"), (dict(height=8193), b"8192"),
                     (dict(struct_size=24), b"struct_size"), (dict(struct_size=32), b"struct_size"),
                     (dict(reference_format=_abi.IMAGE_RGBA8_SRGB), b"reference_format"), (dict(reference_format=7), b"reference_format"),
                     (dict(background_color=(0.0, float("nan"), 0.0, 1.0)), b"finite"), (dict(background_color=(0.0, 0.0, 0.0, float("inf"))), b"finite")):
        assert host(**kw) == INVALID and word in lib.nrs_last_error(), (kw, lib.nrs_last_error())
    # the device calls: what is refused before a context is looked at
    p = _abi.ImageMetricsParams()
    assert lib.nrs_image_metrics(None, None, 3, 2, P(img), P(rf), C.byref(p), C.addressof(res), None, None) == INVALID and b"NULL" in lib.nrs_last_error()
    assert lib.nrs_dataset_image_metrics(None, 0, None, P(img), C.byref(p), C.addressof(res), None, None) == INVALID and b"NULL" in lib.nrs_last_error()
    s = _abi.MetricsSummary()
    assert lib.nrs_image_metrics_summary_host(None, 1, C.byref(s)) == INVALID
    assert lib.nrs_image_metrics_summary_host(C.addressof(res), 1, None) == INVALID
    assert lib.nrs_image_metrics_summary_host(C.addressof(res), 0, C.byref(s)) == INVALID


@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (2, 5), (5, 7), (37, 53)])
def test_reflect_blur_against_scipy(shape):
    """pins the reflect rule of metrics_ref (and with it of the header), including axes shorter than the blur's reach"""
    ndimage = pytest.importorskip("scipy.ndimage")
    a = np.random.default_rng(shape[0] * 100 + shape[1]).random(shape)
    want = ndimage.convolve1d(ndimage.convolve1d(a, ref.K, axis=0), ref.K, axis=1)
    assert float(np.abs(ref.blur(a) - want).max()) <= 1e-11
    for n, want_index in ((1, [0, 0, 0, 0, 0]), (2, [1, 0, 0, 1, 1, 0]), (3, [1, 0, 0, 1, 2, 2, 1])):   # indices -2 .. n + 1: (b a | a b c | c b)
        assert ref.reflect_index(np.arange(-2, n + 2), n).tolist() == want_index


@pytest.mark.parametrize("shape", SHAPES)
def test_host_twin_against_the_float64_restatement(built, shape):
    from nerfshop_amd import runtime
    worst = np.zeros(3)
    for color_space in (ref.COLOR_LINEAR, ref.COLOR_SRGB):
        for dtype in (np.float16, np.float32):
            image, reference = ref.make_images(*shape, rgba=color_space == ref.COLOR_SRGB)
            reference = reference.astype(dtype)
            background = (0.0, 0.0, 0.0, 1.0) if dtype == np.float16 else (0.2, 0.4, 0.6, 1.0)
            rec, ssim_map, sq_map = runtime.image_metrics_host(image, reference, color_space=color_space, background=background, want_maps=True)
            want = ref.metrics(image, reference.astype(f32), color_space, background)
            what = f"{shape} colour space {color_space} {np.dtype(dtype).name}"
            worst = np.maximum(worst, ref.check_against_ref(rec, ssim_map, sq_map, want, what))
            ref.check_sums_against_maps(rec, ssim_map, sq_map, what)
            again = runtime.image_metrics_host(image, reference, color_space=color_space, background=background)[0]
            assert again.tobytes() == rec.tobytes(), "the record does not depend on the maps being asked for"
    print(f"{shape}: worst |d ssim| {worst[0]:.3e} mse rel {worst[1]:.3e} ssim map {worst[2]:.3e}")


def test_non_finite_pixels_count_as_the_definition_says(built):
    """a NaN in the rendered image is A = 0; +inf is A = 1; -inf is A = 0; a NaN in the reference makes that channel's squared error 0"""
    from nerfshop_amd import runtime
    image = np.full((3, 4, 4), 0.5, f32)
    reference = np.full((3, 4, 4), 0.5, f32)
    image[0, 0, 0], image[1, 1, 1], image[2, 2, 2] = np.nan, np.inf, -np.inf
    reference[0, 3, 1] = np.nan
    rec, ssim_map, sq_map = runtime.image_metrics_host(image, reference, want_maps=True)
    R = float(ref.linear_to_srgb(0.5))
    want = np.zeros((3, 4))
    want[0, 0], want[1, 1], want[2, 2] = R * R / 3, (1 - R) ** 2 / 3, R * R / 3
    assert np.abs(sq_map - want).max() < 1e-6 and np.isfinite(ssim_map).all() and math.isfinite(float(rec["ssim"]))


def test_identical_images(built):
    from nerfshop_amd import runtime
    image, _ = ref.make_images(37, 53)
    image = np.nan_to_num(image, nan=0.3, posinf=2.0)
    for reference in (image, image.astype(np.float16)):
        rendered = reference.astype(f32)
        rec = runtime.image_metrics_host(rendered, reference)[0]
        assert float(rec["mse"]) == 0.0 and float(rec["psnr"]) == math.inf and float(rec["ssim"]) == 1.0
        assert int(rec["sum_sq_err"]) == 0 and int(rec["sum_ssim"]) == 37 * 53 << 32


def test_summary_against_the_five_formulas(built):
    from nerfshop_amd import _abi, runtime
    recs = np.zeros(4, _abi.METRICS_RECORD_DTYPE)
    recs["mse"] = [1e-3, 4e-5, 2.5e-2, 7e-4]
    recs["ssim"] = [0.91, 0.993, 0.42, 0.88]
    recs["psnr"] = (-10.0 * np.log10(recs["mse"].astype(np.float64))).astype(f32)
    for case in (recs, recs[:1]):
        got, want = runtime.metrics_summary(case), ref.summary(case["mse"], case["ssim"], case["psnr"])
        assert got["n_views"] == len(case)
        for k in ("psnr_mean", "psnr_min", "psnr_max", "ssim_mean", "psnr_avgmse"):
            assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (k, got[k], want[k])
    assert abs(runtime.metrics_summary(recs)["psnr_avgmse"] - (-10.0 * math.log10(np.mean(recs["mse"].astype(np.float64))))) < 1e-12
    recs["mse"][1], recs["psnr"][1], recs["ssim"][1] = 0.0, np.inf, 1.0   # a view rendered exactly
    got = runtime.metrics_summary(recs)
    assert got["psnr_mean"] == math.inf and got["psnr_max"] == math.inf and abs(got["psnr_min"] - float(recs["psnr"][2])) < 1e-12
    assert math.isfinite(got["psnr_avgmse"]) and abs(got["ssim_mean"] - float(recs["ssim"].astype(np.float64).mean())) < 1e-12
    recs["mse"][:], recs["psnr"][:] = 0.0, np.inf
    assert runtime.metrics_summary(recs)["psnr_avgmse"] == math.inf
    assert runtime.metrics_summary(recs.view(np.uint8).reshape(4, 32))["n_views"] == 4, "the records as the device returns them: [n, 32] bytes"


def _check_program_inputs():
    """the inputs of tests/metrics_host_check.cpp, case by case in its order: (width, height, half, color_space, image, reference)"""
    state = 12345
    def units(n):   # noqa: E306
        nonlocal state
        out = np.empty(n, np.uint32)
        for i in range(n):
            state = (state * 1664525 + 1013904223) & 0xffffffff
            out[i] = state >> 8
        return out.astype(f32) * f32(1.0 / 16777216.0)
    for width, height in ((53, 37), (1, 1), (3, 2)):
        for half in (False, True):
            for color_space in (0, 1):
                n = 4 * width * height
                image = units(n) * f32(1.25) - f32(0.125)
                reference = f32(0.0625) + (units(n) * f32(512.0)).astype(np.int32).astype(f32) / f32(1024.0)
                yield width, height, half, color_space, image.reshape(height, width, 4), reference.reshape(height, width, 4)


def test_host_twin_under_sanitizers(built, tmp_path):
    """The stand-alone program, built with the host compiler under -fsanitize=address,undefined and run on the CPU: clean, and its sums are the library's, bit for bit
    (two compilers, one header, glibc's powf, no contraction)."""
    from nerfshop_amd import runtime
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    flags = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror"]
    trial = tmp_path / "trial.cpp"   # does this compiler have the sanitizers' runtimes at all?  Asked with a program that cannot fail for another reason
    trial.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx, *flags, str(trial), "-o", str(tmp_path / "trial")], capture_output=True, text=True).returncode != 0:
        pytest.skip("the host compiler cannot build an empty program under -fsanitize=address,undefined")
    exe = str(tmp_path / "metrics_host_check")
    build = subprocess.run([cxx, *flags, os.path.join(ROOT, "tests", "metrics_host_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0 and run.stderr == "" and run.stdout.rstrip().endswith("all ok"), (run.returncode, run.stderr[-2000:])
    lines = run.stdout.splitlines()
    for line, (width, height, half, color_space, image, reference) in zip(lines, _check_program_inputs()):
        words = line.split()
        assert words[0] == f"{width}x{height}" and words[-1] == "ok", line
        rec = runtime.image_metrics_host(image, reference.astype(np.float16) if half else reference, color_space=color_space, background=(0.25, 0.0, 1.0, 1.0))[0]
        assert (int(words[4]), int(words[6])) == (int(rec["sum_sq_err"]), int(rec["sum_ssim"])), line
