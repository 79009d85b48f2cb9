"""Image metrics in float64 numpy, restated from the definition in include/nrs.h ("image metrics"): the reference blend, the sRGB-encoded clipped values, the squared
error, the SSIM of a luminance under a separable 5-tap blur with a `reflect` boundary, the fixed-point sums and the record.  The blur is this file's own (an index
table per axis); test_metrics_host.py pins it against scipy.ndimage.convolve1d.  Also the generator of the test images."""
import math

import numpy as np

K = np.array([0.120078, 0.233881, 0.292082, 0.233881, 0.120078])
SCALE = 2.0 ** 32
COLOR_LINEAR, COLOR_SRGB = 0, 1


def linear_to_srgb(x):
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(x > 0.0031308, 1.055 * np.power(np.maximum(x, 0.0), 1.0 / 2.4) - 0.055, 12.92 * x)


def srgb_to_linear(x):
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(x > 0.04045, np.power((np.maximum(x, 0.0) + 0.055) / 1.055, 2.4), x / 12.92)


def reflect_index(i, n):
    """index i of an axis of length n under scipy's `reflect`: j = i mod 2n; j < n ? j : 2n - 1 - j"""
    j = np.mod(i, 2 * n)
    return np.where(j < n, j, 2 * n - 1 - j)


def blur_axis(a, axis):
    n = a.shape[axis]
    out = np.zeros_like(a, dtype=np.float64)
    for k in range(5):
        out += K[k] * np.take(a, reflect_index(np.arange(n) + k - 2, n), axis=axis)
    return out


def blur(a):
    return blur_axis(blur_axis(np.asarray(a, np.float64), 0), 1)


def reference_image(ref_rgba, color_space=COLOR_LINEAR, background=(0.0, 0.0, 0.0, 1.0)):
    """step 1: the linear reference rgb from the stored RGBA (linear, premultiplied)"""
    rf = np.asarray(ref_rgba).astype(np.float64)
    if color_space != COLOR_SRGB:
        return rf[..., :3]
    a = rf[..., 3:4]
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.where(a != 0, rf[..., :3] / np.where(a != 0, a, 1.0), 0.0)
    c = linear_to_srgb(c) * a + (1.0 - a) * np.asarray(background, np.float64)[:3]
    return srgb_to_linear(c)


def encoded(image, ref_rgba, color_space=COLOR_LINEAR, background=(0.0, 0.0, 0.0, 1.0)):
    """step 2: (A, R)"""
    with np.errstate(invalid="ignore"):
        A = np.clip(linear_to_srgb(np.asarray(image).astype(np.float64)[..., :3]), 0.0, 1.0)
        A = np.where(np.isfinite(A), A, 0.0)
        R = np.clip(linear_to_srgb(reference_image(ref_rgba, color_space, background)), 0.0, 1.0)
    return A, R


def luminance(a):
    a = np.power(a, 0.4545454545)
    return 0.2126 * a[..., 0] + 0.7152 * a[..., 1] + 0.0722 * a[..., 2]


def ssim_map(A, R):
    la, lb = luminance(A), luminance(R)
    mA, mB = blur(la), blur(lb)
    sA, sB, sAB = blur(la * la) - mA * mA, blur(lb * lb) - mB * mB, blur(la * lb) - mA * mB
    with np.errstate(invalid="ignore", divide="ignore"):
        s = (2.0 * mA * mB + 1e-4) / (mA * mA + mB * mB + 1e-4) * (2.0 * sAB + 9e-4) / (sA + sB + 9e-4)
    return np.where(np.isfinite(s), s, 0.0)


def fixed(x):
    """step 5: an array of terms -> their sum as a Python int"""
    return int(np.rint(np.asarray(x, np.float64) * SCALE).astype(np.int64).sum(dtype=np.int64))


def record(sum_sq_err, sum_ssim, n):
    """step 6 from the two integer sums: (mse, ssim, psnr) as float32"""
    mse = np.float32(sum_sq_err / SCALE / (3.0 * n))
    ssim = np.float32(sum_ssim / SCALE / n)
    with np.errstate(divide="ignore"):
        psnr = np.float32(-10.0 * np.log10(np.float64(mse))) if mse != 0 else np.float32(np.inf)
    return mse, ssim, psnr


def metrics(image, ref_rgba, color_space=COLOR_LINEAR, background=(0.0, 0.0, 0.0, 1.0)):
    """-> dict: sum_sq_err, sum_ssim, n_pixels, mse, ssim, psnr, ssim_map [H, W], sq_err_map [H, W] (the mean of the three channels)"""
    A, R = encoded(image, ref_rgba, color_space, background)
    with np.errstate(invalid="ignore"):
        e = (A - R) ** 2
    e = np.where(np.isfinite(e), e, 0.0)
    s = ssim_map(A, R)
    n = s.size
    out = {"sum_sq_err": fixed(e), "sum_ssim": fixed(s), "n_pixels": n, "ssim_map": s, "sq_err_map": e.mean(axis=-1)}
    out["mse"], out["ssim"], out["psnr"] = record(out["sum_sq_err"], out["sum_ssim"], n)
    return out


def summary(mse, ssim, psnr):
    """run.py's totals over per-view values"""
    mse, ssim, psnr = (np.asarray(v, np.float64) for v in (mse, ssim, psnr))
    mean_mse = mse.mean()
    with np.errstate(divide="ignore"):
        avg = -10.0 * np.log10(mean_mse) if mean_mse != 0 else np.inf
    return {"psnr_mean": psnr.mean(), "psnr_min": psnr.min(), "psnr_max": psnr.max(), "ssim_mean": ssim.mean(), "psnr_avgmse": avg, "n_views": len(mse)}


def make_images(height, width, seed=0, rgba=False):
    """(image [H, W, 4] float32, reference [H, W, 4] float32): smooth colour, the top left quarter black, the bottom right quarter a flat 0.25, noise on top, values
    below 0 and above 1 in both, one NaN and one inf in the rendered image (where it has room).  rgba: the reference's alpha is 0, 0.5 and 1 in vertical bands and
    its colour premultiplied (for the sRGB blend); otherwise alpha is 1."""
    rng = np.random.default_rng(seed * 7919 + height * 131 + width)
    y, x = np.mgrid[0:height, 0:width]
    u, v = x / max(width - 1, 1), y / max(height - 1, 1)
    smooth = np.stack([0.15 + 0.7 * u, 0.1 + 0.8 * v, 0.5 + 0.4 * np.sin(3.0 * u + 2.0 * v)], -1)
    ref = smooth + 0.05 * rng.standard_normal((height, width, 3))
    ref[: height // 2, : width // 2] = 0.0
    ref[height - height // 2:, width - width // 2:] = 0.25
    img = ref + 0.03 * rng.standard_normal((height, width, 3))
    img[: height // 2, : width // 2] = np.abs(0.002 * rng.standard_normal((height // 2, width // 2, 3)))
    flat = img.reshape(-1, 3)
    n = flat.shape[0]
    if n >= 6:
        flat[n // 3] = (-0.2, 1.7, 0.5)
        ref.reshape(-1, 3)[n // 3 + 1] = (1.3, -0.1, 0.9)
    if n >= 12:
        flat[n // 2, 1] = np.nan
        flat[n // 2 + 2, 0] = np.inf
    alpha = np.ones((height, width, 1))
    if rgba:
        alpha[:, : width // 3] = 0.0
        alpha[:, width // 3: 2 * width // 3 + (1 if width < 3 else 0)] = 0.5
        ref = ref * alpha
    image = np.concatenate([img, rng.random((height, width, 1))], -1).astype(np.float32)
    reference = np.concatenate([ref, alpha], -1).astype(np.float32)
    return image, reference


# ---- what the CPU and the GPU tests both hold a record and its maps to (the origin of the bars: tests/test_metrics_host.py) -------------------------------------------
SSIM_BAR, MSE_BAR, MAP_BAR = 2e-5, 1e-5, 1e-3


def check_against_ref(rec, ssim_map, sq_map, want, what):
    """the bars of this file on one record and its maps; returns the three distances"""
    d_ssim = abs(float(rec["ssim"]) - float(want["ssim"]))
    d_mse = abs(float(rec["mse"]) - float(want["mse"])) / max(float(want["mse"]), 1e-30)
    d_map = float(np.abs(ssim_map.astype(np.float64) - want["ssim_map"]).max())
    print(f"{what}: |d ssim| {d_ssim:.3e}  mse rel {d_mse:.3e}  ssim map {d_map:.3e}  (ssim {float(rec['ssim']):.6f} psnr {float(rec['psnr']):.4f})")
    assert int(rec["n_pixels"]) == want["n_pixels"], what
    assert d_ssim <= SSIM_BAR, (what, d_ssim)
    assert d_mse <= MSE_BAR, (what, d_mse)
    assert d_map <= MAP_BAR, (what, d_map)
    assert float(np.abs(sq_map.astype(np.float64) - want["sq_err_map"]).max()) <= 1e-6, what   # three float32 operations on values <= 1
    if math.isfinite(float(want["psnr"])):
        assert abs(float(rec["psnr"]) - float(want["psnr"])) <= 10.0 / math.log(10.0) * MSE_BAR + 1e-5, what
    return d_ssim, d_mse, d_map


def check_sums_against_maps(rec, ssim_map, sq_map, what):
    n = ssim_map.size
    assert int(rec["sum_ssim"]) == fixed(ssim_map), what
    assert abs(int(rec["sum_sq_err"]) - fixed(3.0 * sq_map.astype(np.float64))) <= 2306 * n, what
    mse, ssim, psnr = record(int(rec["sum_sq_err"]), int(rec["sum_ssim"]), n)
    assert np.float32(rec["mse"]) == mse and np.float32(rec["ssim"]) == ssim, what
    assert np.float32(rec["psnr"]) == psnr or abs(float(rec["psnr"]) - float(psnr)) <= 1e-5 * abs(float(psnr)), what
