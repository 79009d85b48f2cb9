"""nrs_edit (nrs_api_edit.cpp): the edit operators a render or a grid refresh maps its samples through."""
import ctypes as C

import numpy as np
import torch

from .. import _abi
from .._abi import NrsError, check
from ._base import Handle, _require_cuda, _stream_handle


def _operator_handles(edit_operators):
    """(a ctypes array of the operators' handles, their number) as the ABI takes a list of nrs_edit: one element at least, null when there is no operator."""
    n = len(edit_operators)
    return (C.c_void_p * max(n, 1))(*[op.h for op in edit_operators]), n


class _EditOperator(Handle):
    """What the two edit operators share (ngp::EditOperator, editing/edit_operator.h:25): the handle, the host description it was made from, and the two maps."""

    _destroy = "nrs_edit_destroy"

    def __init__(self, ctx, host):
        super().__init__(ctx.lib)
        self.ctx = ctx
        self.host = host  # keeps the numpy arrays alive
        self.n_vertices = self.n_tets = 0

    def map_rays(self, stream, nerf_coords, empty_mask):
        _require_cuda(nerf_coords, torch.float32, "nerf_coords")
        _require_cuda(empty_mask, torch.uint8, "empty_mask")
        if nerf_coords.dim() != 2 or nerf_coords.shape[1] != 7 or empty_mask.numel() < nerf_coords.shape[0]:
            raise NrsError("map_rays expects coords [n, 7] and an empty mask of n bytes")
        check(self.lib.nrs_edit_map_rays(self.h, _stream_handle(stream), nerf_coords.shape[0], nerf_coords.data_ptr(), empty_mask.data_ptr()))

    def map_positions(self, stream, nerf_pos, empty_mask):
        _require_cuda(nerf_pos, torch.float32, "nerf_pos")
        _require_cuda(empty_mask, torch.uint8, "empty_mask")
        if nerf_pos.dim() != 2 or nerf_pos.shape[1] < 3 or empty_mask.numel() < nerf_pos.shape[0]:
            raise NrsError("map_positions expects positions [n, >=3] and an empty mask of n bytes")
        check(self.lib.nrs_edit_map_positions(self.h, _stream_handle(stream), nerf_pos.shape[0], nerf_pos.data_ptr(), nerf_pos.shape[1],
                                              empty_mask.data_ptr()))


class CageDeformation(_EditOperator):
    """One cage-deformation edit operator; owns its GPU tables (tet_mesh.h:80-94)."""

    def __init__(self, ctx, desc, cage_edit, device_authoring=False):
        super().__init__(ctx, cage_edit)
        mesh = cage_edit.tet_mesh_struct(device_authoring) if device_authoring else cage_edit.tet_mesh_struct()
        self.n_vertices, self.n_tets = int(mesh.n_vertices), int(mesh.n_tets)
        check(self.lib.nrs_edit_create(ctx.h, C.byref(desc), C.byref(mesh), C.byref(self.h)))

    # ---- the per-gizmo-move chain on the device (nrs.h "next" row f1) ----
    def set_mvc(self, weights):
        """Cage::compute_mvc's [V, n_cage_vertices] weights, uploaded once."""
        w = np.ascontiguousarray(weights, np.float32)
        if w.ndim != 2 or w.shape[0] != self.n_vertices:
            raise NrsError("set_mvc expects weights [n_vertices, n_cage_vertices]")
        check(self.lib.nrs_edit_set_mvc(self.h, w.ctypes.data, w.shape[1]))

    def update_cage(self, stream, cage_vertices):
        """Cage::interpolate_with_mvc + post_update_vertices + build_tet_grid + update_local_rotations for a moved cage."""
        c = np.ascontiguousarray(cage_vertices, np.float32)
        check(self.lib.nrs_edit_update_cage(self.h, _stream_handle(stream), c.ctypes.data, c.shape[0]))

    def update_vertices(self, stream, vertices):
        v = np.ascontiguousarray(vertices, np.float32)
        check(self.lib.nrs_edit_update_vertices(self.h, _stream_handle(stream), v.ctypes.data, v.shape[0]))

    def poisson_interpolate(self, stream, inside_density, outside_density, inside_shs, outside_shs, residual_amplitude=1.0, gamma=None):
        """GrowingSelection::interpolate_poisson_boundary: per-cage-vertex membrane terms -> the operator's per-tet-vertex ones (on the device)."""
        i_d, o_d = np.ascontiguousarray(inside_density, np.float32), np.ascontiguousarray(outside_density, np.float32)
        i_s, o_s = np.ascontiguousarray(inside_shs, np.float32).reshape(-1, 27), np.ascontiguousarray(outside_shs, np.float32).reshape(-1, 27)
        g = np.ascontiguousarray(gamma, np.float32) if gamma is not None else None
        check(self.lib.nrs_edit_poisson_interpolate(self.h, _stream_handle(stream), g.ctypes.data if g is not None else None, i_d.size, i_d.ctypes.data, o_d.ctypes.data,
                                                    i_s.ctypes.data, o_s.ctypes.data, float(residual_amplitude)))

    def download_poisson(self, n_vertices):
        sh, od, rd = np.zeros((n_vertices, 27), np.float32), np.zeros(n_vertices, np.float32), np.zeros(n_vertices, np.float32)
        check(self.lib.nrs_edit_download_poisson(self.h, sh.ctypes.data, od.ctypes.data, rd.ctypes.data))
        return sh, od, rd

    def lut_size(self):
        n, m = C.c_uint32(), C.c_uint32()
        check(self.lib.nrs_edit_lut_size(self.h, C.byref(n), C.byref(m)))
        return n.value, m.value

    def download(self, rotations=True):
        """-> dict(vertices, lut_offsets, lut_idx, rotations | None, original_bitfield, bbox)"""
        n_idx, _ = self.lut_size()
        out = dict(vertices=np.zeros((self.n_vertices, 3), np.float32), lut_offsets=np.zeros(_abi.N_LUT_CELLS + 1, np.uint32),
                   lut_idx=np.zeros(max(n_idx, 1), np.uint32), rotations=np.zeros((self.n_tets, 9), np.float32) if rotations else None,
                   original_bitfield=np.zeros(_abi.BITFIELD_BYTES, np.uint8), bbox=np.zeros(6, np.float32))
        check(self.lib.nrs_edit_download(self.h, out["vertices"].ctypes.data, out["lut_offsets"].ctypes.data, out["lut_idx"].ctypes.data,
                                         out["rotations"].ctypes.data if rotations else None, out["original_bitfield"].ctypes.data,
                                         out["bbox"].ctypes.data))
        out["lut_idx"] = out["lut_idx"][:n_idx]
        return out


class AffineDuplication(CageDeformation):
    """AffineDuplication edit operator (editing/affine_duplication.h): shares map_rays / map_positions with the cage operator."""

    def __init__(self, ctx, desc, op):
        # a CageDeformation without a cage: its constructor is the shared one, and the cage methods stay reachable (the library refuses them on this operator)
        _EditOperator.__init__(self, ctx, op)
        check(self.lib.nrs_edit_create_affine(ctx.h, C.byref(desc), C.byref(op), C.byref(self.h)))
