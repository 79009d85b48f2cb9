"""nrs_dataset (nrs_api_dataset.cpp): posed images on the device and the rays of a training step."""
import ctypes as C

import numpy as np
import torch

from .. import _abi
from .._abi import NrsError, check
from ._base import Handle, _device, _ptr, _stream_handle


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

    def rays(self, n_rays, n_rays_total, rng, snap=True, random_bg=True, stream=None, want_pixels=True):
        """The rays of one training step (nrs_dataset_rays).  rng = (state, inc) of the step's generator (nrs_rng_seed / nrs_rng_advance); n_rays_total: the rays of
        the steps before.  snap and random_bg default to the reference's Testbed initialisers, snap_to_pixel_centers = true and random_bg_color = true
        (include/neural-graphics-primitives/testbed.h:584 and :581).  Returns CUDA tensors (rays [n, 6] f32, jitter [n] f32, target_rgba [n, 4] f32,
        background [n, 3] f32 sRGB-encoded or None without random_bg, pixels [n, 2] int32 (image, x + y * width) or None)."""
        n = int(n_rays)
        dev = _device(self.ctx)
        p = _abi.DatasetRaysParams()
        p.n_rays_total, p.rng_state, p.rng_inc = int(n_rays_total) & 0xffffffff, int(rng[0]), int(rng[1])
        p.snap_to_pixel_centers, p.random_bg_color = int(bool(snap)), int(bool(random_bg))
        rays = torch.empty((n, 6), dtype=torch.float32, device=dev)
        jitter = torch.empty(n, dtype=torch.float32, device=dev)
        target = torch.empty((n, 4), dtype=torch.float32, device=dev)
        background = torch.empty((n, 3), dtype=torch.float32, device=dev) if random_bg else None
        pixels = torch.empty((n, 2), dtype=torch.int32, device=dev) if want_pixels else None
        check(self.lib.nrs_dataset_rays(self.h, _stream_handle(stream), C.byref(p), n, rays.data_ptr(), jitter.data_ptr(), target.data_ptr(),
                                        _ptr(background), _ptr(pixels)))
        return rays, jitter, target, background, pixels

    def mark_untrained(self, network, clear_visible=True, stream=None):
        """mark_untrained_density_grid on the network's density grid: cells no camera sees become -1 (and stay so through every later grid update), seen cells 0 where
        clear_visible or their sign disagrees; the bitfield is rebuilt.  Waits for the stream, like every bitfield rebuild."""
        check(self.lib.nrs_dataset_mark_untrained(network.h, self.h, 1 if clear_visible else 0, _stream_handle(stream)))
