"""nrs_selection (nrs_api_selection.cpp): region growing over the density grid, the morphology of its bitfield and the fine mesh."""
import ctypes as C

import numpy as np
import torch

from .. import _abi
from .._abi import NrsError, check
from ._base import Handle, _require_cuda, _stream_handle
from .mesh import Mesh


class GrowingSelection(Handle):
    """nrs_selection: RegionGrowing (region_growing.cu) with GrowingSelection's dilate / erode / extract_fine_mesh (growing_selection.cu:2083-2162).  Growing and the
    accessors are host-only; dilate, erode and extract_fine_mesh need a Context (ctx may be None until then)."""

    _destroy = "nrs_selection_destroy"

    def __init__(self, ctx, density_grid, max_cascade=0, lib=None):
        super().__init__(lib if lib is not None else (ctx.lib if ctx is not None else _abi.load()))
        self.ctx = ctx
        grid = np.ascontiguousarray(density_grid, np.float32).reshape(-1)
        check(self.lib.nrs_selection_create(grid.ctypes.data, grid.size, int(max_cascade), C.byref(self.h)))
        self.use_morphological = True   # m_use_morphological
        self.selection_mesh = None      # the Mesh of the last extract_fine_mesh

    def reset_growing(self, selected_cells, growing_level):
        cells = np.ascontiguousarray(selected_cells, np.uint32).reshape(-1)
        check(self.lib.nrs_selection_reset(self.h, cells.ctypes.data, cells.size, int(growing_level)))

    def grow_region(self, density_threshold=0.01, growing_level=None, growing_steps=10000):
        """grow_region in Manual mode; the reference's defaults (growing_selection.h: m_density_threshold 0.01, m_growing_steps 10000) -> entries popped"""
        n = C.c_uint32()
        level = self.growing_level if growing_level is None else int(growing_level)
        check(self.lib.nrs_selection_grow(self.h, float(density_threshold), level, int(growing_steps), C.byref(n)))
        return n.value

    def upscale_growing(self):
        check(self.lib.nrs_selection_upscale(self.h))

    def set_structuring_elements(self, dilation=(_abi.SE_CUBE, 2), erosion=(_abi.SE_SPHERE, 2)):
        check(self.lib.nrs_selection_set_structuring_elements(self.h, int(dilation[0]), int(dilation[1]), int(erosion[0]), int(erosion[1])))

    def _state(self):
        level, n_cells, n_queue, closed = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_int()
        check(self.lib.nrs_selection_state(self.h, C.byref(level), C.byref(n_cells), C.byref(n_queue), C.byref(closed)))
        return level.value, n_cells.value, n_queue.value, bool(closed.value)

    growing_level = property(lambda self: self._state()[0])
    queue_size = property(lambda self: self._state()[2])
    performed_closing = property(lambda self: self._state()[3])

    @property
    def selection_cell_idx(self):
        out = np.zeros(self._state()[1], np.uint32)
        check(self.lib.nrs_selection_get_cells(self.h, out.ctypes.data, None))
        return out

    @property
    def selection_points(self):
        out = np.zeros((self._state()[1], 3), np.float32)
        check(self.lib.nrs_selection_get_cells(self.h, None, out.ctypes.data))
        return out

    @property
    def selection_grid_bitfield(self):
        out = np.zeros(_abi.BITFIELD_BYTES, np.uint8)
        check(self.lib.nrs_selection_get_bitfield(self.h, out.ctypes.data))
        return out

    def dilate(self, stream=None):
        check(self.lib.nrs_selection_dilate(self.ctx.h, _stream_handle(stream), self.h))

    def erode(self, stream=None):
        check(self.lib.nrs_selection_erode(self.ctx.h, _stream_handle(stream), self.h))

    def extract_fine_mesh(self, stream=None):
        """extract_fine_mesh: the closing first when use_morphological and it has not been done since the last growth -> Mesh (also kept as self.selection_mesh)"""
        h = C.c_void_p()
        check(self.lib.nrs_selection_fine_mesh(self.ctx.h, _stream_handle(stream), self.h, 1 if self.use_morphological else 0, C.byref(h)))
        if self.selection_mesh is not None:
            self.selection_mesh.close()
        self.selection_mesh = Mesh(self.lib, h)
        return self.selection_mesh


def bitfield_morph(ctx, bitfield, level, op, se_type, radius, out=None, stream=None):
    """nrs_bitfield_morph: dilation (_abi.MORPH_DILATE) or erosion of one level of a uint8 CUDA tensor [BITFIELD_BYTES] -> a new one (other levels zero)"""
    _require_cuda(bitfield, torch.uint8, "bitfield")
    if out is None:
        out = torch.empty_like(bitfield)
    _require_cuda(out, torch.uint8, "out")
    if bitfield.numel() != _abi.BITFIELD_BYTES or out.numel() != _abi.BITFIELD_BYTES:
        raise NrsError("bitfield_morph: a bitfield holds BITFIELD_BYTES bytes")
    check(ctx.lib.nrs_bitfield_morph(ctx.h, _stream_handle(stream), bitfield.data_ptr(), int(level), int(op), int(se_type), int(radius), out.data_ptr()))
    return out


def bitfield_morph_host(bitfield, level, op, se_type, radius):
    """nrs_bitfield_morph_host: the same on a numpy uint8 array, on one CPU thread"""
    b = np.ascontiguousarray(bitfield, np.uint8).reshape(-1)
    if b.size != _abi.BITFIELD_BYTES:
        raise NrsError("bitfield_morph_host: a bitfield holds BITFIELD_BYTES bytes")
    out = np.empty_like(b)
    check(_abi.load().nrs_bitfield_morph_host(b.ctypes.data, int(level), int(op), int(se_type), int(radius), out.ctypes.data))
    return out
