"""The render surface and the display step over it (nrs_api_display.cpp): accumulate, accumulate_spp, tonemap."""
import ctypes as C

import torch

from .. import _abi
from .._abi import NrsError, check
from ._base import _require_cuda, _stream_handle


class RenderBuffer:
    """frame_buffer(): f32x4 premultiplied linear RGBA [H, W, 4]; depth_buffer(): f32 [H, W]; spp(): Sobol sample index."""

    def __init__(self, width, height, device="cuda:0", with_steps=False):
        self.width, self.height = int(width), int(height)
        self._frame = torch.zeros((self.height, self.width, 4), dtype=torch.float32, device=device)
        self._depth = torch.zeros((self.height, self.width), dtype=torch.float32, device=device)
        self._steps = torch.zeros((self.height, self.width), dtype=torch.int32, device=device) if with_steps else None
        self._spp = 0
        self._accumulate = None   # the running mean: made by the first accumulate call
        self._slabs = None        # spp_slabs()' tensors
        self._color_space, self._tonemap_curve = 0, 0

    def in_resolution(self):
        return (self.width, self.height)

    def frame_buffer(self):
        return self._frame

    def depth_buffer(self):
        return self._depth

    def steps_buffer(self):
        return self._steps

    def spp(self):
        return self._spp

    def set_spp(self, v):
        self._spp = int(v)

    def _ensure_accumulate(self):
        if self._accumulate is None:
            self._accumulate = torch.zeros_like(self._frame)
        return self._accumulate

    def _check_frames(self, frames):
        _require_cuda(frames, torch.float32, "frames")
        if frames.dim() != 4 or tuple(frames.shape[1:]) != (self.height, self.width, 4):
            raise ValueError(f"frames must be [K, {self.height}, {self.width}, 4], got {tuple(frames.shape)}")
        return int(frames.shape[0])

    def accumulate(self, ctx, stream=None, color_space=0):
        """CudaRenderBuffer::accumulate (render_buffer.cu:540): the frame buffer joins the running mean of this view's spp frames; spp() counts them."""
        acc = self._ensure_accumulate()
        check(ctx.lib.nrs_accumulate(ctx.h, _stream_handle(stream), self.width, self.height, self._frame.data_ptr(), acc.data_ptr(), int(self._spp), int(color_space)))
        self._spp += 1
        return acc

    def spp_slabs(self, spp_count):
        """Frame [K, H, W, 4], depth [K, H, W] and (with_steps) steps [K, H, W] slabs for Testbed.render_nerf_spp: allocated on first use, the frame slabs cleared on every call."""
        k = int(spp_count)
        if self._slabs is None or self._slabs[0].shape[0] != k:
            dev = self._frame.device
            self._slabs = (torch.zeros((k, self.height, self.width, 4), dtype=torch.float32, device=dev),
                           torch.zeros((k, self.height, self.width), dtype=torch.float32, device=dev),
                           torch.zeros((k, self.height, self.width), dtype=torch.int32, device=dev) if self._steps is not None else None)
        else:
            self._slabs[0].zero_()
        return self._slabs

    def accumulate_spp(self, ctx, frames, stream=None, color_space=0):
        """The K slabs of `frames` [K, H, W, 4] (Testbed.render_nerf_spp) join the running mean in sample order, bit-equal to K accumulate() calls, in one pass
        over the accumulate buffer (nrs_accumulate_spp); spp() advances by K."""
        k = self._check_frames(frames)
        acc = self._ensure_accumulate()
        check(ctx.lib.nrs_accumulate_spp(ctx.h, _stream_handle(stream), self.width, self.height, frames.data_ptr(), self.width * self.height, k,
                                         acc.data_ptr(), int(self._spp), int(color_space)))
        self._spp += k
        return acc

    def set_color_space(self, color_space):
        """CudaRenderBuffer::set_color_space (render_buffer.h:233): the EColorSpace of the accumulate buffer, read by tonemap() and accumulate_spp_tonemap()."""
        if int(color_space) != self._color_space:   # (a change resets the accumulation, as there)
            self._color_space = int(color_space)
            self._spp = 0

    def set_tonemap_curve(self, curve):
        """CudaRenderBuffer::set_tonemap_curve (render_buffer.h:233): ETonemapCurve, 0 Identity, 1 ACES, 2 Hable, 3 Reinhard."""
        if int(curve) != self._tonemap_curve:
            self._tonemap_curve = int(curve)
            self._spp = 0

    _TONEMAP_FORMATS = {"rgba32f": _abi.TONEMAP_RGBA32F, "rgba8": _abi.TONEMAP_RGBA8}

    def _tonemap_params(self, exposure, background, output_color_space, fmt, clamp_output):
        if fmt not in self._TONEMAP_FORMATS:
            raise ValueError(f"fmt is 'rgba32f' or 'rgba8', got {fmt!r}")
        t = _abi.TonemapParams()
        t.exposure = float(exposure)
        t.background_color[:] = [float(v) for v in background]
        t.color_space = self._color_space
        t.output_color_space = int(output_color_space)
        t.tonemap_curve = self._tonemap_curve
        t.clamp_output = 1 if clamp_output else 0
        t.output_format = self._TONEMAP_FORMATS[fmt]
        return t

    def _tonemap_output(self, fmt):
        if fmt == "rgba8":
            return torch.empty((self.height, self.width, 4), dtype=torch.uint8, device=self._frame.device)
        return torch.empty((self.height, self.width, 4), dtype=torch.float32, device=self._frame.device)

    def tonemap(self, ctx, exposure=0.0, background=(0.0, 0.0, 0.0, 0.0), output_color_space=1, fmt="rgba32f", stream=None, clamp_output=False):
        """CudaRenderBuffer::tonemap(exposure, background_color, output_color_space, stream) (render_buffer.cu:562) of the accumulate buffer: background, exposure, the
        curve of set_tonemap_curve, the output's colour space.  Returns a new tensor [H, W, 4]: float32 for fmt "rgba32f", uint8 (R, G, B, A; clamped) for "rgba8"."""
        if self._accumulate is None:
            raise NrsError("RenderBuffer.tonemap: nothing has been accumulated")
        t = self._tonemap_params(exposure, background, output_color_space, fmt, clamp_output)
        out = self._tonemap_output(fmt)
        check(ctx.lib.nrs_tonemap(ctx.h, _stream_handle(stream), self.width, self.height, self._accumulate.data_ptr(), C.byref(t), out.data_ptr()))
        return out

    def accumulate_spp_tonemap(self, ctx, frames, exposure=0.0, background=(0.0, 0.0, 0.0, 0.0), output_color_space=1, fmt="rgba32f", stream=None, clamp_output=False):
        """accumulate_spp(ctx, frames, color_space of set_color_space) followed by tonemap(...), in one pass over the accumulate buffer (nrs_accumulate_spp_tonemap):
        bit-equal to the pair.  spp() advances by K; returns the output tensor as tonemap() does."""
        k = self._check_frames(frames)
        acc = self._ensure_accumulate()
        t = self._tonemap_params(exposure, background, output_color_space, fmt, clamp_output)
        out = self._tonemap_output(fmt)
        check(ctx.lib.nrs_accumulate_spp_tonemap(ctx.h, _stream_handle(stream), self.width, self.height, frames.data_ptr(), self.width * self.height, k,
                                                 acc.data_ptr(), int(self._spp), C.byref(t), out.data_ptr()))
        self._spp += k
        return out

    def accumulate_buffer(self):
        return self._accumulate

    def clear_frame(self, stream=None):
        self._frame.zero_()
        self._depth.zero_()
