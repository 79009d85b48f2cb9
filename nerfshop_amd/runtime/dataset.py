"""nrs_dataset (nrs_api_dataset.cpp): posed images on the device and the rays of a training step."""
import ctypes as C

import numpy as np
import torch

from .. import _abi
from .._abi import NrsError, check
from ._base import Handle, _device, _ptr, _stream_handle


def error_map_resolution(steps_between, rays_per_batch, n_images, image_resolution):
    """nrs_error_map_resolution: one axis of the error map's resolution as train_nerf picks it, clamped into [2, min(image_resolution, 1024)].  Host only."""
    return int(_abi.load().nrs_error_map_resolution(int(steps_between) & 0xffffffff, int(rays_per_batch) & 0xffffffff, int(n_images), int(image_resolution)))


def error_map_cdfs_host(data):
    """nrs_error_map_cdfs_host: (cdf_x_cond_y [n, res_y, res_x], cdf_y [n, res_y], cdf_img [n], pmf_img [n]) from a float32 error map [n, res_y, res_x], with the
    expressions and the order of Dataset.error_map_build_cdfs.  Host only."""
    a = np.ascontiguousarray(data, dtype=np.float32)
    if a.ndim != 3:
        raise NrsError("error_map_cdfs_host: data must be [n_images, res_y, res_x]")
    n, res_y, res_x = a.shape
    cx, cy = np.zeros((n, res_y, res_x), np.float32), np.zeros((n, res_y), np.float32)
    ci, pi = np.zeros(n, np.float32), np.zeros(n, np.float32)
    check(_abi.load().nrs_error_map_cdfs_host(n, res_y, res_x, a.ctypes.data, cx.ctypes.data, cy.ctypes.data, ci.ctypes.data, pi.ctypes.data))
    return cx, cy, ci, pi


class Dataset(Handle):
    """Posed images on the device (nrs_dataset_*): n_images images of one resolution as fp16 RGBA, linear and premultiplied (NerfDataset::images_data), and one camera
    record per image.  rays() is the first half of generate_training_samples_nerf: the pixels a training step looks at, their rays and the colours they should have."""

    _destroy = "nrs_dataset_destroy"
    _FORMATS = {np.dtype(np.uint8): (_abi.IMAGE_RGBA8_SRGB, torch.uint8), np.dtype(np.float32): (_abi.IMAGE_RGBA32F_LINEAR, torch.float32),
                np.dtype(np.float16): (_abi.IMAGE_RGBA16F_LINEAR, torch.float16)}

    def __init__(self, ctx, n_images, width, height):
        super().__init__(ctx.lib)
        self.ctx = ctx
        self.n_images, self.width, self.height = int(n_images), int(width), int(height)
        self._cameras = {}   # index -> a copy of the TrainingCamera set_camera sent (get_camera: what Testbed.evaluate renders with)
        check(self.lib.nrs_dataset_create(ctx.h, self.n_images, self.width, self.height, C.byref(self.h)))

    def set_image(self, index, pixels, flags=0, mask_color=0, stream=None):
        """Image `index` from pixels [height, width, 4]: uint8 = sRGB with straight alpha (from_rgba32: linearised and premultiplied on the device; flags
        _abi.IMAGE_WHITE_TRANSPARENT / _BLACK_TRANSPARENT, a pixel whose bytes equal a non-zero mask_color is masked away), float32 = linear premultiplied, rounded to
        fp16 (from_fullp), float16 = copied as it is.  A numpy array or a CUDA tensor."""
        shape = (self.height, self.width, 4)
        if isinstance(pixels, torch.Tensor) and pixels.is_cuda:
            fmt = [f for f, t in self._FORMATS.values() if t == pixels.dtype]
            if not fmt or tuple(pixels.shape) != shape or not pixels.is_contiguous():
                raise NrsError(f"Dataset.set_image: pixels must be a contiguous {shape} uint8, float32 or float16 tensor")
            check(self.lib.nrs_dataset_set_image(self.h, int(index), fmt[0], pixels.data_ptr(), 1, int(flags), int(mask_color), _stream_handle(stream)))
            return
        a = np.ascontiguousarray(pixels.numpy() if isinstance(pixels, torch.Tensor) else pixels)
        if a.dtype not in self._FORMATS or a.shape != shape:
            raise NrsError(f"Dataset.set_image: pixels must be a {shape} uint8, float32 or float16 array")
        check(self.lib.nrs_dataset_set_image(self.h, int(index), self._FORMATS[a.dtype][0], a.ctypes.data, 0, int(flags), int(mask_color), _stream_handle(stream)))

    def get_image(self, index):
        """Image `index` as the dataset holds it: [height, width, 4] float16 on the host (synchronous)."""
        out = np.empty((self.height, self.width, 4), dtype=np.float16)
        check(self.lib.nrs_dataset_get_image(self.h, int(index), out.ctypes.data))
        return out

    def set_camera(self, index, camera):
        """Camera `index`: an _abi.TrainingCamera (matrices 3 x 4 column-major, focal length in pixels, principal point as a fraction of the image)."""
        if not isinstance(camera, _abi.TrainingCamera):
            raise NrsError("Dataset.set_camera: camera must be a TrainingCamera")
        check(self.lib.nrs_dataset_set_camera(self.h, int(index), C.byref(camera)))
        self._cameras[int(index)] = _abi.TrainingCamera.from_buffer_copy(camera)

    def rays(self, n_rays, n_rays_total, rng, snap=True, random_bg=True, stream=None, want_pixels=True, by_error=None):
        """The rays of one training step (nrs_dataset_rays).  rng = (state, inc) of the step's generator (nrs_rng_seed / nrs_rng_advance); n_rays_total: the rays of
        the steps before.  snap and random_bg default to the reference's Testbed initialisers, snap_to_pixel_centers = true and random_bg_color = true
        (include/neural-graphics-primitives/testbed.h:584 and :581).  Returns CUDA tensors (rays [n, 6] f32, jitter [n] f32, target_rgba [n, 4] f32,
        background [n, 3] f32 sRGB-encoded or None without random_bg, pixels [n, 2] int32 (image, x + y * width) or None).
        by_error=(images, pixels) goes through nrs_dataset_rays_ex instead -- images drawn from cdf_img, pixels from cdf_y / cdf_x_cond_y, each behind its switch;
        (False, False) draws what the plain call draws -- and returns two more tensors: xy [n, 2] f32 (after snapping) and pdf [n] f32."""
        n = int(n_rays)
        dev = _device(self.ctx)
        p = _abi.DatasetRaysParams() if by_error is None else _abi.DatasetRaysExParams()
        p.n_rays_total, p.rng_state, p.rng_inc = int(n_rays_total) & 0xffffffff, int(rng[0]), int(rng[1])
        p.snap_to_pixel_centers, p.random_bg_color = int(bool(snap)), int(bool(random_bg))
        rays = torch.empty((n, 6), dtype=torch.float32, device=dev)
        jitter = torch.empty(n, dtype=torch.float32, device=dev)
        target = torch.empty((n, 4), dtype=torch.float32, device=dev)
        background = torch.empty((n, 3), dtype=torch.float32, device=dev) if random_bg else None
        pixels = torch.empty((n, 2), dtype=torch.int32, device=dev) if want_pixels else None
        if by_error is None:
            check(self.lib.nrs_dataset_rays(self.h, _stream_handle(stream), C.byref(p), n, rays.data_ptr(), jitter.data_ptr(), target.data_ptr(),
                                            _ptr(background), _ptr(pixels)))
            return rays, jitter, target, background, pixels
        p.sample_images_by_error, p.sample_pixels_by_error = int(bool(by_error[0])), int(bool(by_error[1]))
        xy = torch.empty((n, 2), dtype=torch.float32, device=dev)
        pdf = torch.empty(n, dtype=torch.float32, device=dev)
        check(self.lib.nrs_dataset_rays_ex(self.h, _stream_handle(stream), C.byref(p), n, rays.data_ptr(), jitter.data_ptr(), target.data_ptr(),
                                           _ptr(background), _ptr(pixels), xy.data_ptr(), pdf.data_ptr()))
        return rays, jitter, target, background, pixels, xy, pdf

    # ---- the training error map (include/nrs.h): cells in 64-bit fixed point, three CDFs, rays(by_error=...) ------------------------------------------------------
    def error_map_resolution(self, steps_between, rays_per_batch):
        """(res_x, res_y) the reference picks for this many steps of this many rays (nrs_error_map_resolution), clamped into what error_map_reset accepts."""
        return tuple(int(self.lib.nrs_error_map_resolution(int(steps_between), int(rays_per_batch), self.n_images, r)) for r in (self.width, self.height))

    def error_map_reset(self, res_x, res_y, stream=None):
        """(Re)allocate and zero the map, n_images x res_y x res_x cells.  Valid CDFs survive."""
        check(self.lib.nrs_dataset_error_map_reset(self.h, int(res_x), int(res_y), _stream_handle(stream)))

    def error_map_set(self, data):
        """The map from a float32 array [n_images, res_y, res_x], each entry quantised as a deposit is.  Synchronous."""
        a = np.ascontiguousarray(data, dtype=np.float32)
        if a.ndim != 3 or a.shape[0] != self.n_images:
            raise NrsError("Dataset.error_map_set: data must be [n_images, res_y, res_x]")
        check(self.lib.nrs_dataset_error_map_set(self.h, a.shape[2], a.shape[1], a.ctypes.data))

    def error_map_get(self, what=_abi.ERROR_MAP_FLOAT):
        """The map (_abi.ERROR_MAP_FLOAT: float32, ERROR_MAP_CELLS: the uint64 cells) or one of the CDFs (ERROR_MAP_CDF_X_COND_Y / _CDF_Y / _CDF_IMG / _PMF_IMG) as a
        flat host array; synchronous.  The map is [n_images, res_y, res_x] at the map's resolution, the CDFs at theirs."""
        count = C.c_size_t(0)
        check(self.lib.nrs_dataset_error_map_get(self.h, int(what), None, C.byref(count)))
        out = np.empty(count.value, dtype=np.uint64 if what == _abi.ERROR_MAP_CELLS else np.float32)
        check(self.lib.nrs_dataset_error_map_get(self.h, int(what), out.ctypes.data, None))
        return out

    def error_map_accumulate(self, n_rays, ray_counter, ray_indices, loss, xy, pixels, pdf=None, loss_weighted=None, stream=None):
        """Deposit the losses of one step (nrs_dataset_error_map_accumulate): ray_counter [>= 1] and ray_indices [n] int32 from training_samples, loss [n] f32 by slot
        from ray_loss, xy [n, 2] f32 / pixels [n, 2] int32 / pdf [n] f32 or None by ray from rays(by_error=...).  loss_weighted: None, or a [n] f32 tensor (loss itself
        is allowed) that receives loss / pdf.  CUDA tensors; nothing waits for the device."""
        n = int(n_rays)
        for t, dtype, numel, name in ((ray_counter, torch.int32, 1, "ray_counter"), (ray_indices, torch.int32, n, "ray_indices"), (loss, torch.float32, n, "loss"),
                                      (xy, torch.float32, 2 * n, "xy"), (pixels, torch.int32, 2 * n, "pixels"), (pdf, torch.float32, n, "pdf"),
                                      (loss_weighted, torch.float32, n, "loss_weighted")):
            if t is None and name in ("pdf", "loss_weighted"):
                continue
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or t.numel() < numel:
                raise NrsError(f"Dataset.error_map_accumulate: {name} must be a contiguous CUDA tensor of {dtype} with at least {numel} elements")
        check(self.lib.nrs_dataset_error_map_accumulate(self.h, _stream_handle(stream), n, ray_counter.data_ptr(), ray_indices.data_ptr(), loss.data_ptr(),
                                                        xy.data_ptr(), pixels.data_ptr(), _ptr(pdf), _ptr(loss_weighted)))

    def error_map_build_cdfs(self, stream=None):
        """cdf_x_cond_y, cdf_y, cdf_img and pmf_img from the map, on the device (nrs_dataset_error_map_build_cdfs); they take the map's resolution and become valid."""
        check(self.lib.nrs_dataset_error_map_build_cdfs(self.h, _stream_handle(stream)))

    def image_metrics(self, index, image, color_space=0, background=(0.0, 0.0, 0.0, 1.0), want_maps=False, out=None, stream=None):
        """nrs_dataset_image_metrics: image [height, width, 4] float32 on the device (linear: an accumulate buffer) against image `index` of the dataset, read where it
        lies.  Returns what metrics.image_metrics returns: (record, ssim_map, sq_err_map); `out` is a row of a caller's [n, 32] uint8 CUDA tensor, so one evaluation
        fills one tensor.  Nothing waits for the device."""
        from . import metrics
        h, w = metrics._check_image(image)
        if (h, w) != (self.height, self.width):
            raise NrsError(f"Dataset.image_metrics: image must be [{self.height}, {self.width}, 4]")
        rec, (ssim_map, sq_map) = metrics._outputs(h, w, image.device, want_maps, out)
        p = metrics.metrics_params(color_space, background)
        check(self.lib.nrs_dataset_image_metrics(self.h, int(index), _stream_handle(stream), image.data_ptr(), C.byref(p), rec.data_ptr(), _ptr(ssim_map), _ptr(sq_map)))
        return rec, ssim_map, sq_map

    def get_camera(self, index):
        """The camera set_camera stored for image `index` (a copy), or None while none has been set."""
        return self._cameras.get(int(index))

    def mark_untrained(self, network, clear_visible=True, stream=None):
        """mark_untrained_density_grid on the network's density grid: cells no camera sees become -1 (and stay so through every later grid update), seen cells 0 where
        clear_visible or their sign disagrees; the bitfield is rebuilt.  Waits for the stream, like every bitfield rebuild."""
        check(self.lib.nrs_dataset_mark_untrained(network.h, self.h, 1 if clear_visible else 0, _stream_handle(stream)))
