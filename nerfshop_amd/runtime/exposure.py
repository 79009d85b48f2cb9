"""nrs_exposure (nrs_api_exposure.cpp): per-image exposure -- the scaled target a training ray is compared with, the exposure's gradient and its Adam step."""
import ctypes as C

import numpy as np
import torch

from .. import _abi
from .._abi import NrsError, check
from ._base import Handle, _device, _ptr, _require_cuda, _stream_handle


class Exposure(Handle):
    """n_images x 3 log2 exposures with their own Adam (the reference's per-image AdamOptimizer: 0.9 / 0.99 / 1e-8), all on the device (nrs_exposure_*).  Fresh
    exposures are all zero: every scale is 1.  One training step, and an update every params.steps_between_updates of them:

        target_by_slot, scale = exposure.targets(ray_indices, counters[:1], pixels, target_rgba)
        ... = net.ray_loss(..., target_by_slot, ..., aux=aux)
        exposure.accumulate(acc_params, counters[:1], ray_indices, numsteps_out, aux, scale, xy_pdf=None)
        exposure.step(loss_scale, lr)          # every 16th step

    A training view is displayed with the tonemap's exposure + get()[view]."""

    _destroy = "nrs_exposure_destroy"
    _DTYPES = {_abi.EXPOSURE_VALUES: np.float32, _abi.EXPOSURE_M: np.float32, _abi.EXPOSURE_V: np.float32, _abi.EXPOSURE_CELLS: np.int64, _abi.EXPOSURE_GRADIENT: np.float32}

    def __init__(self, ctx, n_images, params=None):
        super().__init__(ctx.lib)
        self.ctx = ctx
        self.n_images = int(n_images)
        if params is not None and not isinstance(params, _abi.ExposureParams):
            raise NrsError("Exposure: params must be an ExposureParams")
        self.params = params if params is not None else _abi.ExposureParams()
        check(self.lib.nrs_exposure_create(ctx.h, self.n_images, C.byref(self.params), C.byref(self.h)))

    def set(self, values=None):
        """The exposures [n_images, 3] f32 from the host, or None for zeros.  Resets the moments, the step count, the cells and the ray count."""
        if values is None:
            check(self.lib.nrs_exposure_set(self.h, None))
            return
        v = np.ascontiguousarray(values.cpu().numpy() if isinstance(values, torch.Tensor) else values)
        if v.dtype != np.float32 or v.size != 3 * self.n_images:
            raise NrsError(f"Exposure.set: expected {3 * self.n_images} float32 values")
        check(self.lib.nrs_exposure_set(self.h, v.ctypes.data))

    def get(self, which=_abi.EXPOSURE_VALUES):
        """_abi.EXPOSURE_VALUES / _M / _V / _GRADIENT as float32 [n_images, 3], EXPOSURE_CELLS as int64; on the host, synchronous."""
        if which not in self._DTYPES:
            raise NrsError("Exposure.get: unknown `which`")
        out = np.empty((self.n_images, 3), dtype=self._DTYPES[which])
        check(self.lib.nrs_exposure_get(self.h, int(which), out.ctypes.data, out.size))
        return out

    def export(self, out=None, stream=None):
        """The exposures as a CUDA tensor [n_images, 3] f32.  Asynchronous."""
        if out is None:
            out = torch.empty((self.n_images, 3), dtype=torch.float32, device=_device(self.ctx))
        _require_cuda(out, torch.float32, "out")
        if out.numel() != 3 * self.n_images:
            raise NrsError(f"Exposure.export: out must hold {3 * self.n_images} floats")
        check(self.lib.nrs_exposure_export(self.h, out.data_ptr(), _stream_handle(stream)))
        return out

    def targets(self, ray_indices, ray_counter, pixels, target_rgba, out=None, stream=None):
        """nrs_exposure_targets: ray_indices [n] int32 and ray_counter [>= 1] int32 from training_samples, pixels [n, 2] int32 (img, pixel) and target_rgba [n, 4]
        f32, both by RAY.  Returns (target [n, 4] f32: (2^exposure * rgb, a), scale [n, 4] int32: the bits of the scale, img), both by SLOT; rows at or past the
        counter and skipped slots are not written (fresh ones are zero).  `out` may bring the two tensors to reuse."""
        _require_cuda(ray_indices, torch.int32, "ray_indices")
        _require_cuda(ray_counter, torch.int32, "ray_counter")
        _require_cuda(pixels, torch.int32, "pixels")
        _require_cuda(target_rgba, torch.float32, "target_rgba")
        if target_rgba.dim() != 2 or target_rgba.shape[1] != 4:
            raise NrsError("Exposure.targets: target_rgba must be [n, 4]")
        n = int(target_rgba.shape[0])
        if ray_indices.numel() < n or ray_counter.numel() < 1 or pixels.numel() != 2 * n:
            raise NrsError("Exposure.targets: ray_indices must be [n], pixels [n, 2] and ray_counter hold one element")
        if out is None:
            out = (torch.zeros((n, 4), dtype=torch.float32, device=target_rgba.device), torch.zeros((n, 4), dtype=torch.int32, device=target_rgba.device))
        target, scale = out
        _require_cuda(target, torch.float32, "target")
        _require_cuda(scale, torch.int32, "scale")
        if tuple(target.shape) != (n, 4) or tuple(scale.shape) != (n, 4):
            raise NrsError("Exposure.targets: out must be ([n, 4] f32, [n, 4] int32)")
        check(self.lib.nrs_exposure_targets(self.h, _stream_handle(stream), n, ray_counter.data_ptr(), ray_indices.data_ptr(), pixels.data_ptr(), target_rgba.data_ptr(),
                                            target.data_ptr(), scale.data_ptr()))
        return target, scale

    def accumulate(self, params, ray_counter, ray_indices, numsteps_out, aux, scale, xy_pdf=None, n_rays=None, stream=None):
        """nrs_exposure_accumulate: deposit the exposure's gradient of one step into the cells.  params: an _abi.ExposureAccumulateParams; numsteps_out [n, 2] int32
        and aux [n, 12] int32 from ray_loss(aux=...), scale from targets(); xy_pdf [n] f32 by ray or None for 1.  n_rays: the normaliser, default
        numsteps_out.shape[0]."""
        if not isinstance(params, _abi.ExposureAccumulateParams):
            raise NrsError("Exposure.accumulate: params must be an ExposureAccumulateParams")
        n = int(numsteps_out.shape[0]) if n_rays is None else int(n_rays)
        for t, dtype, numel, name in ((ray_counter, torch.int32, 1, "ray_counter"), (ray_indices, torch.int32, n, "ray_indices"), (numsteps_out, torch.int32, 2 * n, "numsteps_out"),
                                      (aux, torch.int32, _abi.RAY_AUX_WORDS * n, "aux"), (scale, torch.int32, 4 * n, "scale")):
            _require_cuda(t, dtype, name)
            if t.numel() < numel:
                raise NrsError(f"Exposure.accumulate: {name} must hold at least {numel} elements")
        if xy_pdf is not None:
            _require_cuda(xy_pdf, torch.float32, "xy_pdf")
            if xy_pdf.numel() < n:
                raise NrsError(f"Exposure.accumulate: xy_pdf must hold at least {n} elements")
        check(self.lib.nrs_exposure_accumulate(self.h, _stream_handle(stream), C.byref(params), n, ray_counter.data_ptr(), ray_indices.data_ptr(), numsteps_out.data_ptr(),
                                               aux.data_ptr(), scale.data_ptr(), _ptr(xy_pdf)))

    def step(self, loss_scale=128.0, lr=_abi.BASE_LEARNING_RATE, stream=None):
        """nrs_exposure_step: Adam on every image from the cells (an image without rays still steps), the renormalisation to zero mean, the cells' reset.  Asynchronous."""
        check(self.lib.nrs_exposure_step(self.h, _stream_handle(stream), float(loss_scale), float(lr)))

    def step_count(self):
        return int(self.lib.nrs_exposure_step_count(self.h))


def exposure_step_host(cells, values, m, v, step_count, loss_scale, lr, params=None):
    """nrs_exposure_step_host: the step's host twin.  cells [n_images, 3] int64, values / m / v [n_images, 3] f32 -> (cells, values, m, v, step_count) after the
    step, as new arrays.  No device."""
    lib = _abi.load()
    params = params if params is not None else _abi.ExposureParams()
    cells = np.array(cells, dtype=np.int64, order="C")
    values, m, v = (np.array(a, dtype=np.float32, order="C") for a in (values, m, v))
    n_images = cells.size // 3
    if cells.size != 3 * n_images or any(a.size != cells.size for a in (values, m, v)):
        raise NrsError("exposure_step_host: the four arrays must hold 3 * n_images elements each")
    t = C.c_uint32(int(step_count))
    check(lib.nrs_exposure_step_host(n_images, C.byref(params), float(loss_scale), float(lr), cells.ctypes.data, values.ctypes.data, m.ctypes.data, v.ctypes.data, C.byref(t)))
    return cells, values, m, v, int(t.value)
