"""Image metrics (nrs_api_metrics.cpp): the squared error and SSIM of scripts/run.py --test_transforms, of a rendered view against a reference image, on the device."""
import ctypes as C

import numpy as np
import torch

from .. import _abi
from .._abi import NrsError, check
from ._base import _ptr, _require_cuda, _stream_handle

RECORD_BYTES = C.sizeof(_abi.ImageMetricsResult)  # 32
_REF_FORMATS = {torch.float16: _abi.IMAGE_RGBA16F_LINEAR, torch.float32: _abi.IMAGE_RGBA32F_LINEAR}
_REF_FORMATS_HOST = {np.dtype(np.float16): _abi.IMAGE_RGBA16F_LINEAR, np.dtype(np.float32): _abi.IMAGE_RGBA32F_LINEAR}


def metrics_params(color_space=0, background=(0.0, 0.0, 0.0, 1.0), reference_format=_abi.IMAGE_RGBA16F_LINEAR):
    p = _abi.ImageMetricsParams()
    p.color_space, p.reference_format = int(color_space), int(reference_format)
    p.background_color[:] = [float(v) for v in background]
    return p


def _check_image(image, name="image"):
    _require_cuda(image, torch.float32, name)
    if image.dim() != 3 or image.shape[2] != 4:
        raise NrsError(f"{name} must be [height, width, 4] float32")
    return int(image.shape[0]), int(image.shape[1])


def _outputs(height, width, device, want_maps, out):
    """The record's tensor (32 bytes of uint8: `out`, a row of a caller's [n, 32] uint8 CUDA tensor, or a new one) and the two maps or (None, None)"""
    if out is None:
        out = torch.empty(RECORD_BYTES, dtype=torch.uint8, device=device)
    elif not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.uint8 or out.numel() != RECORD_BYTES or not out.is_contiguous():
        raise NrsError("out must be a contiguous CUDA tensor of 32 uint8 (a row of a [n, 32] tensor)")
    maps = (torch.empty((height, width), dtype=torch.float32, device=device), torch.empty((height, width), dtype=torch.float32, device=device)) if want_maps else (None, None)
    return out, maps


def records_from_bytes(raw):
    """A [n, 32] (or [32]) uint8 tensor or array of records -> a numpy record array with the fields of nrs_image_metrics_result.  A CUDA tensor is copied (synchronous)."""
    if isinstance(raw, torch.Tensor):
        raw = raw.cpu().numpy()
    return np.ascontiguousarray(raw, np.uint8).reshape(-1, RECORD_BYTES).view(_abi.METRICS_RECORD_DTYPE).reshape(-1)


def image_metrics(ctx, image, reference, color_space=0, background=(0.0, 0.0, 0.0, 1.0), want_maps=False, out=None, stream=None):
    """nrs_image_metrics: image [H, W, 4] float32 (linear: an accumulate buffer) against reference [H, W, 4] float16 or float32 (linear, premultiplied), CUDA tensors.
    Returns (record, ssim_map, sq_err_map): the record as 32 uint8 on the device (`out` when given; records_from_bytes reads it), the maps [H, W] float32 or None
    without want_maps.  Nothing waits for the device."""
    h, w = _check_image(image)
    if not isinstance(reference, torch.Tensor) or not reference.is_cuda or reference.dtype not in _REF_FORMATS or not reference.is_contiguous() or \
            tuple(reference.shape) != (h, w, 4):
        raise NrsError(f"reference must be a contiguous [{h}, {w}, 4] float16 or float32 CUDA tensor")
    rec, (ssim_map, sq_map) = _outputs(h, w, image.device, want_maps, out)
    p = metrics_params(color_space, background, _REF_FORMATS[reference.dtype])
    check(ctx.lib.nrs_image_metrics(ctx.h, _stream_handle(stream), w, h, image.data_ptr(), reference.data_ptr(), C.byref(p), rec.data_ptr(), _ptr(ssim_map), _ptr(sq_map)))
    return rec, ssim_map, sq_map


def image_metrics_host(image, reference, color_space=0, background=(0.0, 0.0, 0.0, 1.0), want_maps=False):
    """nrs_image_metrics_host: the CPU twin on numpy arrays (image [H, W, 4] float32, reference [H, W, 4] float16 or float32) -> (record, ssim_map, sq_err_map), the
    record a numpy record (fields of nrs_image_metrics_result).  No GPU."""
    img = np.ascontiguousarray(image, np.float32)
    ref = np.ascontiguousarray(reference)
    if img.ndim != 3 or img.shape[2] != 4 or ref.shape != img.shape or ref.dtype not in _REF_FORMATS_HOST:
        raise NrsError("image_metrics_host: image [H, W, 4] float32 and reference [H, W, 4] float16 or float32")
    h, w = img.shape[:2]
    res = _abi.ImageMetricsResult()
    ssim_map, sq_map = (np.empty((h, w), np.float32), np.empty((h, w), np.float32)) if want_maps else (None, None)
    p = metrics_params(color_space, background, _REF_FORMATS_HOST[ref.dtype])
    check(_abi.load().nrs_image_metrics_host(w, h, img.ctypes.data, ref.ctypes.data, C.byref(p), C.addressof(res), ssim_map.ctypes.data if want_maps else None,
                                             sq_map.ctypes.data if want_maps else None))
    return records_from_bytes(np.frombuffer(bytes(res), np.uint8))[0], ssim_map, sq_map


def metrics_summary(records):
    """nrs_image_metrics_summary_host: run.py's totals over the records (a numpy record array, or [n, 32] uint8) -> a dict: psnr_mean, psnr_min, psnr_max, ssim_mean,
    psnr_avgmse (the PSNR of the mean MSE), n_views."""
    a = np.ascontiguousarray(records)
    if a.dtype == np.uint8:
        a = records_from_bytes(a)
    a = np.ascontiguousarray(a.astype(_abi.METRICS_RECORD_DTYPE, copy=False)).reshape(-1)
    s = _abi.MetricsSummary()
    check(_abi.load().nrs_image_metrics_summary_host(a.ctypes.data, a.size, C.byref(s)))
    return {"psnr_mean": s.psnr_mean, "psnr_min": s.psnr_min, "psnr_max": s.psnr_max, "ssim_mean": s.ssim_mean, "psnr_avgmse": s.psnr_avgmse, "n_views": int(s.n_views)}
