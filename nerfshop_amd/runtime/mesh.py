"""nrs_mesh (nrs_api_mesh.cpp): a triangle mesh on the device, from marching cubes over a density field."""
import ctypes as C
import os

import numpy as np
import torch

from .._abi import NrsError, check
from ._base import Handle, _float3, _require_cuda, _stream_handle, _uint3


class Mesh(Handle):
    """nrs_mesh: a triangle mesh on the device (m_mesh's verts, vert_normals, vert_colors, verts_smoothed, indices)"""

    _destroy = "nrs_mesh_destroy"

    def __init__(self, lib, handle):
        super().__init__(lib, handle)
        nv, npad, nt = C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(lib.nrs_mesh_counts(handle, C.byref(nv), C.byref(npad), C.byref(nt)))
        self.n_verts, self.n_verts_padded, self.n_tris = nv.value, npad.value, nt.value
        ptrs = [C.c_void_p() for _ in range(5)]
        check(lib.nrs_mesh_device(handle, *[C.byref(p) for p in ptrs]))
        self.d_verts, self.d_normals, self.d_colors, self.d_smoothed, self.d_indices = [p.value for p in ptrs]

    def download(self):
        """-> (V [n_padded, 3], N [n_padded, 3] not normalised, C [n_padded, 3] or None, S [n_padded, 4], F uint32 [n_tris, 3]) numpy arrays"""
        n, t = self.n_verts_padded, self.n_tris
        V, N, S, F = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 4), np.float32), np.zeros((t, 3), np.uint32)
        Cc = np.zeros((n, 3), np.float32) if self.d_colors else None
        check(self.lib.nrs_mesh_download(self.h, V.ctypes.data, N.ctypes.data, Cc.ctypes.data if Cc is not None else None, S.ctypes.data, F.ctypes.data))
        return V, N, Cc, S, F

    def save(self, filename, scale=1.0, offset=(0.0, 0.0, 0.0)):
        V, N, Cc, _, F = self.download()
        if Cc is None:
            Cc = np.zeros_like(V)
        check(self.lib.nrs_mesh_write(os.fsencode(filename), V.shape[0], V.ctypes.data, N.ctypes.data, Cc.ctypes.data, F.shape[0], F.ctypes.data, float(scale),
                                      C.byref(_float3(offset))))


def mesh_from_density(ctx, density, aabb_min, aabb_max, thresh, stream=None):
    """marching_cubes_gpu + compute_mesh_1ring on a caller's field: a float32 CUDA tensor [rz, ry, rx] (what Testbed.get_density_on_grid returns) -> Mesh"""
    _require_cuda(density, torch.float32, "density")
    if density.dim() != 3 or not density.is_contiguous():
        raise NrsError("mesh_from_density: density must be a contiguous [rz, ry, rx] tensor")
    rz, ry, rx = density.shape
    h = C.c_void_p()
    check(ctx.lib.nrs_mesh_from_density(ctx.h, _stream_handle(stream), C.byref(_uint3((rx, ry, rz))), C.byref(_float3(aabb_min)),
                                        C.byref(_float3(aabb_max)), float(thresh), density.data_ptr(), C.byref(h)))
    return Mesh(ctx.lib, h)
