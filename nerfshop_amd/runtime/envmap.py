"""nrs_envmap (nrs_api_envmap.cpp): the trainable environment map -- the background a training ray sees, its gradient and its optimiser step."""
import ctypes as C

import numpy as np
import torch

from .. import _abi
from .._abi import NrsError, check
from ._base import Handle, _device, _float3, _ptr, _require_cuda, _stream_handle


class Envmap(Handle):
    """res_x x res_y RGBA float texels with their own Adam (base.json's envmap block by default), all on the device (nrs_envmap_*).  A fresh map is all zeros.  The
    training loss reads the live texels; export(ema=True) is what a Testbed renders with (Testbed.envmap).  One training step:

        bg_linear, footprint = envmap.background(rays, ray_indices, counters[:1], background=bg_by_slot)
        ... = net.ray_loss(..., background_linear=bg_linear, aux=aux)
        envmap.accumulate(acc_params, counters[:1], numsteps_out, aux, bg_linear, footprint)
        envmap.step(loss_scale, lr)
    """

    _destroy = "nrs_envmap_destroy"
    _DTYPES = {_abi.ENVMAP_TEXELS: np.float32, _abi.ENVMAP_EMA: np.float32, _abi.ENVMAP_GRADIENT: np.float32, _abi.ENVMAP_CELLS: np.int64}

    def __init__(self, ctx, res_x, res_y, params=None):
        super().__init__(ctx.lib)
        self.ctx = ctx
        self.res_x, self.res_y = int(res_x), int(res_y)
        if params is not None and not isinstance(params, _abi.AdamParams):
            raise NrsError("Envmap: params must be an AdamParams")
        self.params = params
        check(self.lib.nrs_envmap_create(ctx.h, self.res_x, self.res_y, None if params is None else C.byref(params), C.byref(self.h)))
        self.n = 4 * self.res_x * self.res_y

    def set_texels(self, texels, stream=None):
        """The live texels [res_y, res_x, 4] f32: a CUDA tensor or a host array.  Resets the optimiser (the EMA becomes the texels), the gradient and the cells."""
        if isinstance(texels, torch.Tensor) and texels.is_cuda:
            _require_cuda(texels, torch.float32, "texels")
            if texels.numel() != self.n:
                raise NrsError(f"Envmap.set_texels: expected {self.n} floats")
            check(self.lib.nrs_envmap_set_texels(self.h, texels.data_ptr(), 1, _stream_handle(stream)))
            return
        t = np.ascontiguousarray(texels.numpy() if isinstance(texels, torch.Tensor) else texels)
        if t.dtype != np.float32 or t.size != self.n:
            raise NrsError(f"Envmap.set_texels: expected {self.n} float32 values")
        check(self.lib.nrs_envmap_set_texels(self.h, t.ctypes.data, 0, _stream_handle(stream)))

    def get(self, which=_abi.ENVMAP_TEXELS):
        """_abi.ENVMAP_TEXELS / ENVMAP_EMA / ENVMAP_GRADIENT as float32 [res_y, res_x, 4], ENVMAP_CELLS as int64; on the host, synchronous."""
        if which not in self._DTYPES:
            raise NrsError("Envmap.get: unknown `which`")
        out = np.empty((self.res_y, self.res_x, 4), dtype=self._DTYPES[which])
        check(self.lib.nrs_envmap_get(self.h, int(which), out.ctypes.data, out.size))
        return out

    def export(self, ema=True, out=None, stream=None):
        """The EMA (or, ema=False, the live) texels as a CUDA tensor [res_y, res_x, 4] f32: what Testbed.envmap takes.  Asynchronous."""
        if out is None:
            out = torch.empty((self.res_y, self.res_x, 4), dtype=torch.float32, device=_device(self.ctx))
        _require_cuda(out, torch.float32, "out")
        if out.numel() != self.n:
            raise NrsError(f"Envmap.export: out must hold {self.n} floats")
        check(self.lib.nrs_envmap_export(self.h, 1 if ema else 0, out.data_ptr(), _stream_handle(stream)))
        return out

    def background(self, rays, ray_indices, ray_counter, background=None, default_background=(0.0, 0.0, 0.0), out=None, stream=None):
        """nrs_envmap_background: rays [n, 6] f32 by ray, ray_indices [n] int32 and ray_counter [>= 1] int32 from training_samples, background [n, 3] f32 by SLOT
        (sRGB-encoded) or None for default_background.  Returns (background_linear [n, 3] f32, footprint [n, 4] int32: tx, ty, the bits of wx, wy), both by slot;
        rows at or past the counter are not written (fresh ones are zero).  `out` may bring the two tensors to reuse."""
        _require_cuda(rays, torch.float32, "rays")
        _require_cuda(ray_indices, torch.int32, "ray_indices")
        _require_cuda(ray_counter, torch.int32, "ray_counter")
        if rays.dim() != 2 or rays.shape[1] != 6:
            raise NrsError("Envmap.background: rays must be [n, 6]")
        n = int(rays.shape[0])
        if ray_indices.numel() < n or ray_counter.numel() < 1:
            raise NrsError("Envmap.background: ray_indices must be [n] and ray_counter hold one element")
        if background is not None:
            _require_cuda(background, torch.float32, "background")
            if tuple(background.shape) != (n, 3):
                raise NrsError("Envmap.background: background must be [n, 3]")
        if out is None:
            out = (torch.zeros((n, 3), dtype=torch.float32, device=rays.device), torch.zeros((n, 4), dtype=torch.int32, device=rays.device))
        bg_linear, footprint = out
        _require_cuda(bg_linear, torch.float32, "background_linear")
        _require_cuda(footprint, torch.int32, "footprint")
        if tuple(bg_linear.shape) != (n, 3) or tuple(footprint.shape) != (n, 4):
            raise NrsError("Envmap.background: out must be ([n, 3] f32, [n, 4] int32)")
        check(self.lib.nrs_envmap_background(self.h, _stream_handle(stream), n, ray_counter.data_ptr(), ray_indices.data_ptr(), rays.data_ptr(), _ptr(background),
                                             C.byref(_float3([float(v) for v in default_background])), bg_linear.data_ptr(), footprint.data_ptr()))
        return bg_linear, footprint

    def accumulate(self, params, ray_counter, numsteps_out, aux, background_linear, footprint, n_rays=None, stream=None):
        """nrs_envmap_accumulate: deposit the envmap's gradient of one step into the cells.  params: an _abi.EnvmapAccumulateParams; numsteps_out [n, 2] int32 and aux
        [n, 12] int32 from ray_loss(aux=...), background_linear and footprint from background().  n_rays: the normaliser, default numsteps_out.shape[0]."""
        if not isinstance(params, _abi.EnvmapAccumulateParams):
            raise NrsError("Envmap.accumulate: params must be an EnvmapAccumulateParams")
        n = int(numsteps_out.shape[0]) if n_rays is None else int(n_rays)
        for t, dtype, numel, name in ((ray_counter, torch.int32, 1, "ray_counter"), (numsteps_out, torch.int32, 2 * n, "numsteps_out"),
                                      (aux, torch.int32, _abi.RAY_AUX_WORDS * n, "aux"), (background_linear, torch.float32, 3 * n, "background_linear"),
                                      (footprint, torch.int32, 4 * n, "footprint")):
            _require_cuda(t, dtype, name)
            if t.numel() < numel:
                raise NrsError(f"Envmap.accumulate: {name} must hold at least {numel} elements")
        check(self.lib.nrs_envmap_accumulate(self.h, _stream_handle(stream), C.byref(params), n, ray_counter.data_ptr(), numsteps_out.data_ptr(), aux.data_ptr(),
                                             background_linear.data_ptr(), footprint.data_ptr()))

    def step(self, loss_scale=1.0, lr=_abi.ENVMAP_LEARNING_RATE, stream=None):
        """nrs_envmap_step: the cells become the float gradient (and zero), then one optimiser step on the texels.  Asynchronous."""
        check(self.lib.nrs_envmap_step(self.h, _stream_handle(stream), float(loss_scale), float(lr)))

    def step_count(self):
        return int(self.lib.nrs_envmap_step_count(self.h))
