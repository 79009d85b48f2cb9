"""nrs_model, the network entry points and the training-ray entry points (nrs_api_model.cpp, nrs_api_network.cpp, nrs_api_train.cpp)."""
import ctypes as C
import os

import numpy as np
import torch

from .. import _abi
from .._abi import NrsError, check
from ._base import Handle, _float3, _ptr, _require_cuda, _stream_handle
from .edits import _operator_handles

DEFAULT_CELL_CACHE_BYTES = 10 << 30  # levels 0..11 of base.json's table (9.2 GB)


class NerfNetwork(Handle):
    """pos-encoding (HashGrid) -> density MLP -> (SH dir-encoding | density features) -> RGB MLP -> extract_density."""

    _destroy = "nrs_model_destroy"

    def __init__(self, ctx, desc, cell_cache_bytes=DEFAULT_CELL_CACHE_BYTES, n_extra_dims=0):
        """cell_cache_bytes: budget of the cell-record cache this HARNESS opts into (nrs_model_set_cell_cache: opt-in at the C-ABI since round 6; never more than a
        quarter of the free HBM); 0 = none.  n_extra_dims: 0, or 3 for a network trained with light directions (nrs_model_create_ex)."""
        super().__init__(ctx.lib)
        self.ctx, self.desc = ctx, desc
        self._n_extra_dims = int(n_extra_dims)
        if self._n_extra_dims:
            check(self.lib.nrs_model_create_ex(ctx.h, C.byref(desc), self._n_extra_dims, C.byref(self.h)))
        else:
            check(self.lib.nrs_model_create(ctx.h, C.byref(desc), C.byref(self.h)))
        if cell_cache_bytes and "NRS_CELL_CACHE_GB" not in os.environ:
            free_b = torch.cuda.mem_get_info(ctx.device)[0]
            try:
                self.set_cell_cache(min(int(cell_cache_bytes), free_b // 4))
            except NrsError:
                self.set_cell_cache(0)  # an optimisation: render without it

    # -- NerfNetwork<T> accessors (nerf_network.h:97-120)
    def padded_output_width(self):
        return 16

    def input_width(self):
        return 7

    def n_extra_dims(self):
        return int(self.lib.nrs_model_n_extra_dims(self.h))

    def n_params(self):
        return int(self.lib.nrs_model_n_params_ex(C.byref(self.desc), self._n_extra_dims))

    def set_light_dir(self, light_dir):
        """m_nerf.light_dir (nrs_model_set_light_dir): normalised at use; what every sample gets that brings no light direction of its own."""
        check(self.lib.nrs_model_set_light_dir(self.h, C.byref(_float3([float(v) for v in light_dir]))))

    def set_params(self, params_fp16):
        """fp16 parameter blob in tiny-cuda-nn order (density | rgb | grid), a host array (numpy uint16/float16)."""
        p = np.ascontiguousarray(params_fp16)
        if p.dtype == np.float16:
            p = p.view(np.uint16)
        if p.dtype != np.uint16:
            raise NrsError("set_params expects fp16 parameters (numpy float16 or their uint16 bits)")
        check(self.lib.nrs_model_set_params(self.h, p.ctypes.data, p.size))

    def set_params_device(self, params_fp16_cuda, stream=None):
        """NerfNetwork::set_params with device pointers: a CUDA tensor of fp16 (or the same bits as int16/uint16) in tcnn order."""
        t = params_fp16_cuda
        if not t.is_cuda or t.element_size() != 2 or not t.is_contiguous():
            raise NrsError("set_params_device expects a contiguous 2-byte CUDA tensor")
        check(self.lib.nrs_model_set_params_device(self.h, t.data_ptr(), t.numel(), _stream_handle(stream)))

    def set_numerics(self, grid_acc=0, mlp_acc=0):
        """tiny-cuda-nn's two unpinned roundings (nrs_model_set_numerics): grid_acc 0 = fp32 sum rounded once, 1 = per-corner fp16 accumulation;
        mlp_acc 0 = fp32 accumulators, 1 = fp16 rounding of the running sum every 16-wide k step."""
        check(self.lib.nrs_model_set_numerics(self.h, int(grid_acc), int(mlp_acc)))

    def set_cell_cache(self, max_bytes):
        """Budget of the cell-record cache (nrs_model_set_cell_cache): 0 drops it; results do not depend on it."""
        check(self.lib.nrs_model_set_cell_cache(self.h, int(max_bytes)))

    def cell_cache(self):
        """(bytes held by the cell records, number of levels they cover)"""
        n = C.c_uint32()
        b = self.lib.nrs_model_cell_cache_bytes(self.h, C.byref(n))
        return int(b), int(n.value)

    def set_sparse_cell_cache(self, mask_bitfield_u8, max_bytes):
        """Sparse brick records for the levels after the dense ones (nrs_model_set_sparse_cell_cache); mask = density-bitfield layout."""
        if mask_bitfield_u8 is None:
            check(self.lib.nrs_model_set_sparse_cell_cache(self.h, None, 0))
            return
        b = np.ascontiguousarray(mask_bitfield_u8, np.uint8)
        assert b.size == _abi.BITFIELD_BYTES
        check(self.lib.nrs_model_set_sparse_cell_cache(self.h, b.ctypes.data, int(max_bytes)))

    def sparse_cell_cache(self):
        """(bytes held by brick tables + records, first sparse level, number of sparse levels)"""
        f, n = C.c_uint32(), C.c_uint32()
        b = self.lib.nrs_model_sparse_cell_cache_bytes(self.h, C.byref(f), C.byref(n))
        return int(b), int(f.value), int(n.value)

    def set_density_bitfield(self, bitfield_u8):
        b = np.ascontiguousarray(bitfield_u8, np.uint8)
        check(self.lib.nrs_model_set_density_bitfield(self.h, b.ctypes.data, b.size))

    def set_density_grid(self, grid_f32):
        g = np.ascontiguousarray(grid_f32, np.float32)
        check(self.lib.nrs_model_set_density_grid(self.h, g.ctypes.data, g.size))

    def get_density_bitfield(self):
        out = np.zeros(_abi.BITFIELD_BYTES, np.uint8)
        check(self.lib.nrs_model_get_density_bitfield(self.h, out.ctypes.data, out.size))
        return out

    def get_march_accelerator(self, which):
        """Test hook: (box12 = min, max, cell, 1/cell; mask bits [32, 32, 32] as bool, z-major) of the marching accelerator."""
        box = np.zeros(12, np.float32)
        mask = np.zeros(1024, np.uint32)
        check(self.lib.nrs_model_get_march_accelerator(self.h, int(which), box.ctypes.data, mask.ctypes.data))
        bits = np.unpackbits(mask.view(np.uint8), bitorder="little").reshape(32, 32, 32).astype(bool)
        return box, bits

    def get_density_grid(self):
        out = np.zeros(_abi.GRID_VOLUME * _abi.GRID_CASCADES, np.float32)
        check(self.lib.nrs_model_get_density_grid(self.h, out.ctypes.data, out.size))
        return out

    def update_density_grid(self, update, edit_operators=(), stream=None):
        """nrs_model_update_density_grid: one refresh of the occupancy from the network, in the space the edit operators deform; `update` is an _abi.GridUpdate."""
        arr, n = _operator_handles(edit_operators)
        check(self.lib.nrs_model_update_density_grid(self.h, arr, n, C.byref(update), _stream_handle(stream)))

    def _records(self, input, output, min_ld, max_ld, message, out_name="output", also=()):
        """The opening of the network methods: f32 records `input` [n, min_ld..max_ld] (max_ld None: no bound) and an fp16 `output`, both contiguous CUDA
        tensors, then the (tensor, dtype, name) triples of `also`.  Returns n; _out_layout tells the output's layout for it."""
        _require_cuda(input, torch.float32, "input")
        _require_cuda(output, torch.float16, out_name)
        for t, dtype, name in also:
            _require_cuda(t, dtype, name)
        if input.dim() != 2 or input.shape[1] < min_ld or (max_ld is not None and input.shape[1] > max_ld):
            raise NrsError(message)
        return input.shape[0]

    def inference_mixed_precision(self, stream, input, output):
        """input: [n, 7] f32 (tcnn: column-major 7 x n).  output: fp16, [16, n_el] (row-major planes, n_el >= n)
        or [n, 16] (column-major / interleaved), as GPUMatrixDynamic's layout selects in the reference."""
        n = self._records(input, output, 7, 7, "NerfNetwork::inference_mixed_precision input must be [n, 7]")
        layout, ld = self._out_layout(output, n)
        check(self.lib.nrs_network_inference(self.h, _stream_handle(stream), n, input.data_ptr(), output.data_ptr(), ld, layout))

    def inference_strided(self, stream, input, output):
        """inference_mixed_precision on [n, ld >= 7] f32 records (nrs_network_inference_strided): with ld >= 10 on a network with light directions, floats 7..9 of
        a record are that sample's already-warped light direction; otherwise the model's light direction is used."""
        n = self._records(input, output, 7, None, "inference_strided input must be a contiguous [n, >= 7] tensor")
        layout, ld = self._out_layout(output, n)
        check(self.lib.nrs_network_inference_strided(self.h, _stream_handle(stream), n, input.data_ptr(), input.shape[1], output.data_ptr(), ld, layout))

    def density(self, stream, input, output):
        """input: [n, ld] f32 with ld in 3..7 (only the position is read); output as above, the density MLP's 16 outputs."""
        n = self._records(input, output, 3, 7, "NerfNetwork::density input must be in column major format ([n, 3..7] here).")
        layout, ld = self._out_layout(output, n)
        check(self.lib.nrs_network_density(self.h, _stream_handle(stream), n, input.data_ptr(), input.shape[1], output.data_ptr(), ld, layout))

    def input_gradient(self, stream, input, output):
        """NerfNetwork::input_gradient(stream, 3, input, output): d density_raw / d position, input [n, >= 3] f32, output [n, 3] f32 (cuda tensors)."""
        _require_cuda(input, torch.float32, "input")
        _require_cuda(output, torch.float32, "output")
        n = input.shape[0]
        assert output.shape == (n, 3) and output.is_contiguous() and input.is_contiguous()
        check(self.lib.nrs_network_input_gradient(self.h, _stream_handle(stream), n, input.data_ptr(), input.shape[1], output.data_ptr()))

    def backward(self, stream, input, dL_doutput, dL_dparams, dL_dinput=None, accumulate=False):
        """NerfNetwork::backward (nrs_network_backward): input [n, >= 7] f32; dL_doutput fp16, [16, n_el] (planes) or [n, 16], rows 0..2 rgb and row 3 density
        (callers scale it by their loss scale); dL_dparams [n_params] f32 in the blob's order, overwritten unless `accumulate`; dL_dinput None or an f32 tensor
        shaped like input (floats 0..2 of a record get dL/dposition, the rest of it zero).  All cuda tensors; base.json's architecture at the default numerics."""
        n = self._records(input, dL_doutput, 7, None, "NerfNetwork::backward input must be a contiguous [n, >= 7] tensor", "dL_doutput",
                          also=((dL_dparams, torch.float32, "dL_dparams"),))
        if dL_dparams.dim() != 1 or not dL_dparams.is_contiguous() or not dL_doutput.is_contiguous():
            raise NrsError("NerfNetwork::backward: dL_dparams must be a contiguous 1-d tensor and dL_doutput contiguous")
        layout, ld = self._out_layout(dL_doutput, n)
        if dL_dinput is not None:
            _require_cuda(dL_dinput, torch.float32, "dL_dinput")
            if tuple(dL_dinput.shape) != tuple(input.shape) or not dL_dinput.is_contiguous():
                raise NrsError("NerfNetwork::backward: dL_dinput must be contiguous and shaped like input")
        check(self.lib.nrs_network_backward(self.h, _stream_handle(stream), n, input.data_ptr(), input.shape[1], dL_doutput.data_ptr(), ld, layout,
                                            dL_dparams.data_ptr(), dL_dparams.numel(), 1 if accumulate else 0, _ptr(dL_dinput)))

    @staticmethod
    def ray_loss_buffers(n_rays, max_samples_compacted, ld=7, dl_planes=False, device=None):
        """The five tensors ray_loss writes, for `n_rays` rows of numsteps and records of `ld` floats: (numsteps_out [n_rays, 2] int32, coords_out [max, ld] f32,
        dL_doutput fp16 [max, 16] or -- dl_planes -- [16, max], loss [n_rays] f32, counter [1] int32).  dL_doutput is zero: ray_loss leaves its rows 4..15 alone."""
        n, cap = int(n_rays), int(max_samples_compacted)
        return (torch.empty((n, 2), dtype=torch.int32, device=device), torch.empty((cap, int(ld)), dtype=torch.float32, device=device),
                torch.zeros((16, cap) if dl_planes else (cap, 16), dtype=torch.float16, device=device),
                torch.empty(n, dtype=torch.float32, device=device), torch.empty(1, dtype=torch.int32, device=device))

    def ray_loss(self, stream, params, numsteps, coords, output, target_rgba, background=None, ray_origins=None, ray_counter=None, n_rays=None,
                 out=None, dl_planes=False, background_linear=None, aux=None):
        """compute_loss_kernel_train_nerf (nrs_ray_loss): composite the samples of every ray, take the loss against target_rgba and write its gradient, compacted.
        params: RayLossParams (max_samples_compacted set).  numsteps [n_rays, 2] u32-as-int32 (count, base); coords [n_samples, >= 7] f32; output fp16 as
        inference wrote it ([16, n_el] or [n_samples, 16]); target_rgba [n_rays, 4] f32; background [n_rays, 3] / ray_origins [n_rays, 3] f32 or None; ray_counter: a
        one-element int32 CUDA tensor (live rays) or None; n_rays: the normaliser, default numsteps.shape[0].
        Returns (numsteps_out [n_rays, 2] int32, coords_out [max, ld] f32, dL_doutput fp16 [max, 16] or -- dl_planes -- [16, max], loss [n_rays] f32, counter [1] int32);
        `out` may bring these five tensors to reuse.  Rows 4..15 of dL_doutput are not written (a fresh one is zero).
        background_linear [n_rays, 3] f32 by slot (Envmap.background) replaces the linearised background; aux [n_rays, 12] int32 receives the slot's record (g[3], T,
        target[3], C[3] as float bits, n, M).  Either goes through nrs_ray_loss_ex; with both None this is nrs_ray_loss."""
        if not isinstance(params, _abi.RayLossParams):
            raise NrsError("ray_loss: params must be a RayLossParams")
        _require_cuda(numsteps, torch.int32, "numsteps")
        _require_cuda(coords, torch.float32, "coords")
        _require_cuda(output, torch.float16, "output")
        _require_cuda(target_rgba, torch.float32, "target_rgba")
        if numsteps.dim() != 2 or numsteps.shape[1] != 2:
            raise NrsError("ray_loss: numsteps must be [n_rays, 2]")
        n = int(numsteps.shape[0]) if n_rays is None else int(n_rays)
        if n > numsteps.shape[0] or tuple(target_rgba.shape) != (numsteps.shape[0], 4):
            raise NrsError("ray_loss: target_rgba must be [n_rays, 4] and n_rays no more than numsteps has rows")
        if coords.dim() != 2 or coords.shape[1] < 7:
            raise NrsError("ray_loss: coords must be a contiguous [n_samples, >= 7] tensor")
        n_samples, ld_in = int(coords.shape[0]), int(coords.shape[1])
        layout, ld_out = self._out_layout(output, n_samples)
        for t, name in ((background, "background"), (ray_origins, "ray_origins")):
            if t is not None:
                _require_cuda(t, torch.float32, name)
                if tuple(t.shape) != (numsteps.shape[0], 3):
                    raise NrsError(f"ray_loss: {name} must be [n_rays, 3]")
        if ray_counter is not None:
            _require_cuda(ray_counter, torch.int32, "ray_counter")
        cap = int(params.max_samples_compacted)
        if cap <= 0:
            raise NrsError("ray_loss: params.max_samples_compacted must be positive")
        if out is None:
            out = self.ray_loss_buffers(numsteps.shape[0], cap, ld_in, dl_planes, coords.device)
        numsteps_out, coords_out, dl, loss, counter = out
        _require_cuda(numsteps_out, torch.int32, "numsteps_out")
        _require_cuda(coords_out, torch.float32, "coords_out")
        _require_cuda(dl, torch.float16, "dL_doutput")
        _require_cuda(loss, torch.float32, "loss")
        _require_cuda(counter, torch.int32, "counter")
        if tuple(numsteps_out.shape) != tuple(numsteps.shape) or tuple(coords_out.shape) != (cap, ld_in) or loss.numel() < numsteps.shape[0] or counter.numel() < 1:
            raise NrsError("ray_loss: an output tensor has the wrong shape")
        dl_layout, ld_dl = self._out_layout(dl, cap)
        args = (self.h, _stream_handle(stream), C.byref(params), n, _ptr(ray_counter), numsteps.data_ptr(),
                n_samples, coords.data_ptr(), ld_in, output.data_ptr(), ld_out, layout, target_rgba.data_ptr(),
                _ptr(background), _ptr(ray_origins),
                numsteps_out.data_ptr(), coords_out.data_ptr(), dl.data_ptr(), ld_dl, dl_layout, loss.data_ptr(), counter.data_ptr())
        if background_linear is None and aux is None:
            check(self.lib.nrs_ray_loss(*args))
            return numsteps_out, coords_out, dl, loss, counter
        if background_linear is not None:
            _require_cuda(background_linear, torch.float32, "background_linear")
            if tuple(background_linear.shape) != (numsteps.shape[0], 3):
                raise NrsError("ray_loss: background_linear must be [n_rays, 3]")
        if aux is not None:
            _require_cuda(aux, torch.int32, "aux")
            if tuple(aux.shape) != (numsteps.shape[0], _abi.RAY_AUX_WORDS):
                raise NrsError("ray_loss: aux must be [n_rays, 12] int32")
        check(self.lib.nrs_ray_loss_ex(*args, _ptr(background_linear), _ptr(aux)))
        return numsteps_out, coords_out, dl, loss, counter

    def training_samples(self, stream, rays, jitter, cone_angle_constant, max_samples, ld=7):
        """generate_training_samples_nerf from the ray on (nrs_training_samples): rays [n, 6] f32 (origin, unit direction), jitter [n] f32 in [0, 1) or None.
        Returns (coords [max_samples, ld] f32, numsteps [n, 2] int32 (count, base) per emitted ray, ray_indices [n] int32, counters [2] int32 = rays emitted,
        sum of all counts).  Rows of numsteps / ray_indices at or past counters[0] are zero (never written)."""
        _require_cuda(rays, torch.float32, "rays")
        if rays.dim() != 2 or rays.shape[1] != 6:
            raise NrsError("training_samples: rays must be [n, 6]")
        n = int(rays.shape[0])
        if jitter is not None:
            _require_cuda(jitter, torch.float32, "jitter")
            if jitter.numel() != n:
                raise NrsError("training_samples: jitter must be [n]")
        if int(max_samples) <= 0 or int(ld) < 7:
            raise NrsError("training_samples: max_samples must be positive and ld >= 7")
        dev = rays.device
        coords = torch.zeros(int(max_samples), int(ld), dtype=torch.float32, device=dev)
        numsteps = torch.zeros(n, 2, dtype=torch.int32, device=dev)
        ray_indices = torch.zeros(n, dtype=torch.int32, device=dev)
        counters = torch.zeros(2, dtype=torch.int32, device=dev)
        check(self.lib.nrs_training_samples(self.h, _stream_handle(stream), n, rays.data_ptr(), _ptr(jitter), float(cone_angle_constant),
                                            int(max_samples), coords.data_ptr(), int(ld), numsteps.data_ptr(), ray_indices.data_ptr(), counters.data_ptr()))
        return coords, numsteps, ray_indices, counters

    def visualize_activation(self, stream, layer, dimension, input, output):
        """Network::visualize_activation: unit `dimension` of forward_activations(layer), input [n, 7] f32, output [n] f32 (cuda tensors)."""
        _require_cuda(input, torch.float32, "input")
        _require_cuda(output, torch.float32, "output")
        n = input.shape[0]
        assert input.shape[1] == 7 and output.shape == (n,) and output.is_contiguous() and input.is_contiguous()
        check(self.lib.nrs_network_visualize_activation(self.h, _stream_handle(stream), int(layer), int(dimension), n, input.data_ptr(), output.data_ptr()))

    def hashgrid_encode(self, stream, input, output):
        _require_cuda(input, torch.float32, "input")
        _require_cuda(output, torch.float16, "output")
        n = input.shape[0]
        if tuple(output.shape) != (n, 32):
            raise NrsError("hashgrid_encode output must be [n, 32]")
        check(self.lib.nrs_hashgrid_encode(self.h, _stream_handle(stream), n, input.data_ptr(), input.shape[1], output.data_ptr()))

    @staticmethod
    def _out_layout(output, n):
        if output.dim() == 2 and output.shape[0] == 16 and output.shape[1] >= n:
            return _abi.LAYOUT_PLANES, int(output.shape[1])
        if output.dim() == 2 and output.shape[1] == 16 and output.shape[0] >= n:
            return _abi.LAYOUT_INTERLEAVED, 16
        raise NrsError("output must be [16, n_el] (planes) or [n, 16] (interleaved) fp16")


def rng_seed(seed):
    """nrs_rng_seed: (state, inc) of pcg32 seeded with `seed` (default_rng_t{seed}).  Host only."""
    st, inc = C.c_uint64(), C.c_uint64()
    _abi.load().nrs_rng_seed(int(seed), C.byref(st), C.byref(inc))
    return st.value, inc.value


def rng_advance(state, inc, delta=_abi.RNG_STEP_DELTA):
    """nrs_rng_advance: pcg32's state after `delta` more steps.  Host only."""
    st = C.c_uint64(int(state))
    _abi.load().nrs_rng_advance(C.byref(st), int(inc), int(delta) & 0xffffffffffffffff)
    return st.value
