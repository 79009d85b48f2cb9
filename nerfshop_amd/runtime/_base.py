"""What every module of the harness shares: the owner of an ABI object and the small ctypes / torch idioms."""
import ctypes as C

import torch

from .._abi import NrsError


class Handle:
    """Owner of one ABI object: the library `lib`, the object's handle `h` (falsy once closed) and `_destroy`, the name of the ABI function that frees it."""

    _destroy = None

    def __init__(self, lib, h=None):
        self.lib, self.h = lib, h if h is not None else C.c_void_p()

    def close(self):
        if self.h:
            getattr(self.lib, self._destroy)(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _stream_handle(stream):
    if stream is None:
        stream = torch.cuda.current_stream()
    if isinstance(stream, torch.cuda.Stream):
        return C.c_void_p(stream.cuda_stream)
    return C.c_void_p(int(stream))


def _require_cuda(t, dtype, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise NrsError(f"{name} must be a CUDA (HIP) tensor")
    if t.dtype != dtype:
        raise NrsError(f"{name} must have dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise NrsError(f"{name} must be contiguous")


def _ptr(t):
    """The device pointer of an optional tensor."""
    return None if t is None else t.data_ptr()


def _float3(v):
    return (C.c_float * 3)(*v)


def _uint3(v):
    return (C.c_uint32 * 3)(*[int(x) for x in v])


def _device(ctx):
    """The torch device string of a Context."""
    return f"cuda:{ctx.device}"
