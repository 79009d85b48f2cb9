"""Host-side mirror of the reference's operator surface for the render path, over the C-ABI of libnrs.so.

Names, argument meaning and error behaviour follow the reference classes so call sites read the same:

    NerfNetwork            <- ngp::NerfNetwork<T> / NerfNetworkFull<T>   include/neural-graphics-primitives/nerf_network.h:86
    CageDeformation        <- ngp::CageDeformation : EditOperator        include/.../editing/edit_operator.h:25, cage_deformation.cu:547
    RenderBuffer           <- ngp::CudaRenderBuffer (frame_buffer / depth_buffer / spp / clear_frame)   render_buffer.h:164
    Testbed.render_nerf    <- Testbed::render_nerf                        src/testbed_nerf.cu:3066

PyTorch is plumbing only: device memory (torch tensors), streams.  All arithmetic happens in the HIP kernels;
there is no CPU path -- a missing library or GPU raises NrsError.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _abi
from ._abi import NrsError, RenderParams, RenderStats, check


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


class Context:
    def __init__(self, device=0):
        self.lib = _abi.load()
        self.h = C.c_void_p()
        check(self.lib.nrs_ctx_create(int(device), C.byref(self.h)))
        self.device = int(device)
        name = C.create_string_buffer(256)
        ncu, hbm = C.c_int(), C.c_size_t()
        check(self.lib.nrs_ctx_device_info(self.h, name, 256, C.byref(ncu), C.byref(hbm)))
        self.device_name, self.n_cus, self.hbm_bytes = name.value.decode(), ncu.value, hbm.value

    def set_lane_teams(self, lanes_per_ray):
        """0 = automatic (default), 1 / 2 / 4 = lanes of a wavefront per ray in render launches, -1 = hybrid, -2 / -3 / -4 = small-launch schedule with
        16- / 32- / 64-pixel packets (nrs_ctx_set_lane_teams)."""
        check(self.lib.nrs_ctx_set_lane_teams(self.h, int(lanes_per_ray)))

    def set_ray_handover(self, enabled):
        """Waves that run out of work take rays from a sibling wave of their workgroup (on by default; nrs_ctx_set_ray_handover)."""
        check(self.lib.nrs_ctx_set_ray_handover(self.h, int(bool(enabled))))

    def ray_handovers(self):
        """(rays moved, hand-overs) of the last render launch that returned statistics."""
        n, k = C.c_uint64(), C.c_uint64()
        check(self.lib.nrs_ctx_ray_handovers(self.h, C.byref(n), C.byref(k)))
        return n.value, k.value

    def render_launches(self):
        """(render-kernel dispatches enqueued through this context, schedule word of the last one) -- nrs_ctx_render_launches."""
        n, sched = C.c_uint64(), C.c_uint32()
        check(self.lib.nrs_ctx_render_launches(self.h, C.byref(n), C.byref(sched)))
        return n.value, sched.value

    def close(self):
        if self.h:
            self.lib.nrs_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


DEFAULT_CELL_CACHE_BYTES = 10 << 30  # levels 0..11 of base.json's table (9.2 GB)


class NerfNetwork:
    """pos-encoding (HashGrid) -> density MLP -> (SH dir-encoding | density features) -> RGB MLP -> extract_density."""

    def __init__(self, ctx, desc, cell_cache_bytes=DEFAULT_CELL_CACHE_BYTES, n_extra_dims=0):
        """cell_cache_bytes: budget of the cell-record cache this HARNESS opts into (nrs_model_set_cell_cache: opt-in at the C-ABI since round 6; never more than a
        quarter of the free HBM); 0 = none.  n_extra_dims: 0, or 3 for a network trained with light directions (nrs_model_create_ex)."""
        self.ctx, self.lib, self.desc = ctx, ctx.lib, desc
        self.h = C.c_void_p()
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
        check(self.lib.nrs_model_set_light_dir(self.h, C.byref((C.c_float * 3)(*[float(v) for v in light_dir]))))

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

    def inference_mixed_precision(self, stream, input, output):
        """input: [n, 7] f32 (tcnn: column-major 7 x n).  output: fp16, [16, n_el] (row-major planes, n_el >= n)
        or [n, 16] (column-major / interleaved), as GPUMatrixDynamic's layout selects in the reference."""
        _require_cuda(input, torch.float32, "input")
        _require_cuda(output, torch.float16, "output")
        if input.dim() != 2 or input.shape[1] != 7:
            raise NrsError("NerfNetwork::inference_mixed_precision input must be [n, 7]")
        n = input.shape[0]
        layout, ld = self._out_layout(output, n)
        check(self.lib.nrs_network_inference(self.h, _stream_handle(stream), n, input.data_ptr(), output.data_ptr(), ld, layout))

    def inference_strided(self, stream, input, output):
        """inference_mixed_precision on [n, ld >= 7] f32 records (nrs_network_inference_strided): with ld >= 10 on a network with light directions, floats 7..9 of
        a record are that sample's already-warped light direction; otherwise the model's light direction is used."""
        _require_cuda(input, torch.float32, "input")
        _require_cuda(output, torch.float16, "output")
        if input.dim() != 2 or input.shape[1] < 7 or not input.is_contiguous():
            raise NrsError("inference_strided input must be a contiguous [n, >= 7] tensor")
        n = input.shape[0]
        layout, ld = self._out_layout(output, n)
        check(self.lib.nrs_network_inference_strided(self.h, _stream_handle(stream), n, input.data_ptr(), input.shape[1], output.data_ptr(), ld, layout))

    def density(self, stream, input, output):
        """input: [n, ld] f32 with ld in 3..7 (only the position is read); output as above, the density MLP's 16 outputs."""
        _require_cuda(input, torch.float32, "input")
        _require_cuda(output, torch.float16, "output")
        if input.dim() != 2 or not (3 <= input.shape[1] <= 7):
            raise NrsError("NerfNetwork::density input must be in column major format ([n, 3..7] here).")
        n = input.shape[0]
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
        _require_cuda(input, torch.float32, "input")
        _require_cuda(dL_doutput, torch.float16, "dL_doutput")
        _require_cuda(dL_dparams, torch.float32, "dL_dparams")
        if input.dim() != 2 or input.shape[1] < 7 or not input.is_contiguous():
            raise NrsError("NerfNetwork::backward input must be a contiguous [n, >= 7] tensor")
        if dL_dparams.dim() != 1 or not dL_dparams.is_contiguous() or not dL_doutput.is_contiguous():
            raise NrsError("NerfNetwork::backward: dL_dparams must be a contiguous 1-d tensor and dL_doutput contiguous")
        n = input.shape[0]
        layout, ld = self._out_layout(dL_doutput, n)
        din = None
        if dL_dinput is not None:
            _require_cuda(dL_dinput, torch.float32, "dL_dinput")
            if tuple(dL_dinput.shape) != tuple(input.shape) or not dL_dinput.is_contiguous():
                raise NrsError("NerfNetwork::backward: dL_dinput must be contiguous and shaped like input")
            din = dL_dinput.data_ptr()
        check(self.lib.nrs_network_backward(self.h, _stream_handle(stream), n, input.data_ptr(), input.shape[1], dL_doutput.data_ptr(), ld, layout,
                                            dL_dparams.data_ptr(), dL_dparams.numel(), 1 if accumulate else 0, din))

    def ray_loss(self, stream, params, numsteps, coords, output, target_rgba, background=None, ray_origins=None, ray_counter=None, n_rays=None,
                 out=None, dl_planes=False):
        """compute_loss_kernel_train_nerf (nrs_ray_loss): composite the samples of every ray, take the loss against target_rgba and write its gradient, compacted.
        params: RayLossParams (max_samples_compacted set).  numsteps [n_rays, 2] u32-as-int32 (count, base); coords [n_samples, >= 7] f32; output fp16 as
        inference wrote it ([16, n_el] or [n_samples, 16]); target_rgba [n_rays, 4] f32; background [n_rays, 3] / ray_origins [n_rays, 3] f32 or None; ray_counter: a
        one-element int32 CUDA tensor (live rays) or None; n_rays: the normaliser, default numsteps.shape[0].
        Returns (numsteps_out [n_rays, 2] int32, coords_out [max, ld] f32, dL_doutput fp16 [max, 16] or -- dl_planes -- [16, max], loss [n_rays] f32, counter [1] int32);
        `out` may bring these five tensors to reuse.  Rows 4..15 of dL_doutput are not written (a fresh one is zero)."""
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
        dev = coords.device
        if out is None:
            out = (torch.empty_like(numsteps), torch.empty(cap, ld_in, dtype=torch.float32, device=dev),
                   torch.zeros((16, cap) if dl_planes else (cap, 16), dtype=torch.float16, device=dev),
                   torch.empty(numsteps.shape[0], dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.int32, device=dev))
        numsteps_out, coords_out, dl, loss, counter = out
        _require_cuda(numsteps_out, torch.int32, "numsteps_out")
        _require_cuda(coords_out, torch.float32, "coords_out")
        _require_cuda(dl, torch.float16, "dL_doutput")
        _require_cuda(loss, torch.float32, "loss")
        _require_cuda(counter, torch.int32, "counter")
        if tuple(numsteps_out.shape) != tuple(numsteps.shape) or tuple(coords_out.shape) != (cap, ld_in) or loss.numel() < numsteps.shape[0] or counter.numel() < 1:
            raise NrsError("ray_loss: an output tensor has the wrong shape")
        dl_layout, ld_dl = self._out_layout(dl, cap)
        check(self.lib.nrs_ray_loss(self.h, _stream_handle(stream), C.byref(params), n, None if ray_counter is None else ray_counter.data_ptr(), numsteps.data_ptr(),
                                    n_samples, coords.data_ptr(), ld_in, output.data_ptr(), ld_out, layout, target_rgba.data_ptr(),
                                    None if background is None else background.data_ptr(), None if ray_origins is None else ray_origins.data_ptr(),
                                    numsteps_out.data_ptr(), coords_out.data_ptr(), dl.data_ptr(), ld_dl, dl_layout, loss.data_ptr(), counter.data_ptr()))
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
        check(self.lib.nrs_training_samples(self.h, _stream_handle(stream), n, rays.data_ptr(), None if jitter is None else jitter.data_ptr(), float(cone_angle_constant),
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

    def close(self):
        if self.h:
            self.lib.nrs_model_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Optimizer:
    """tiny-cuda-nn's Adam (per-parameter step counts, zero-gradient skip, L2 on the matrix weights) with the EMA of base.json, one fused HIP kernel per step
    (nrs_optimizer_*).  Optimizer(ctx, n_params=..., n_matrix=...) keeps an fp16 array of its own; Optimizer(ctx, network=net) is bound to a NerfNetwork: a step
    writes the network's resident hash table in place and refreshes its MLP fragments on the same stream, so the next forward pass reads the new parameters with no
    copy.  The network must outlive the optimiser."""

    _DTYPES = {_abi.OPT_MASTER: np.float32, _abi.OPT_M: np.float32, _abi.OPT_V: np.float32, _abi.OPT_STEPS: np.uint32, _abi.OPT_EMA: np.float32,
               _abi.OPT_PARAMS_FP16: np.float16}

    def __init__(self, ctx, n_params=None, n_matrix=0, network=None, params=None):
        self.ctx, self.lib, self.network = ctx, ctx.lib, network
        self.params = params if params is not None else _abi.AdamParams()
        if not isinstance(self.params, _abi.AdamParams):
            raise NrsError("Optimizer: params must be an AdamParams")
        self.h = C.c_void_p()
        if network is not None:
            check(self.lib.nrs_optimizer_create_for_model(network.h, C.byref(self.params), C.byref(self.h)))
        else:
            if n_params is None:
                raise NrsError("Optimizer: give n_params (and n_matrix) or a network")
            check(self.lib.nrs_optimizer_create(ctx.h, int(n_params), int(n_matrix), C.byref(self.params), C.byref(self.h)))
        nm = C.c_size_t()
        self.n_params = int(self.lib.nrs_optimizer_n_params(self.h, C.byref(nm)))
        self.n_matrix = int(nm.value)

    def set_weights(self, weights_f32, stream=None):
        """The fp32 master weights: a CUDA tensor or a host array of n_params float32.  Resets m, v, the step counts and the EMA."""
        if isinstance(weights_f32, torch.Tensor) and weights_f32.is_cuda:
            _require_cuda(weights_f32, torch.float32, "weights")
            if weights_f32.numel() != self.n_params:
                raise NrsError(f"Optimizer.set_weights: expected {self.n_params} weights")
            check(self.lib.nrs_optimizer_set_weights(self.h, weights_f32.data_ptr(), 1, _stream_handle(stream)))
            return
        w = np.ascontiguousarray(weights_f32.numpy() if isinstance(weights_f32, torch.Tensor) else weights_f32)
        if w.dtype != np.float32 or w.size != self.n_params:
            raise NrsError(f"Optimizer.set_weights: expected {self.n_params} float32 weights")
        check(self.lib.nrs_optimizer_set_weights(self.h, w.ctypes.data, 0, _stream_handle(stream)))

    def step(self, grad, loss_scale=1.0, lr=_abi.BASE_LEARNING_RATE, zero_grad=False, stream=None):
        """One step on grad [n_params] f32 (a CUDA tensor, any 4-byte alignment: a view into a larger buffer is fine), the gradient of loss_scale x the loss.
        zero_grad: the kernel clears every non-zero entry it read, so the next backward pass can accumulate into the same buffer.  Asynchronous."""
        _require_cuda(grad, torch.float32, "grad")
        if grad.numel() != self.n_params:
            raise NrsError(f"Optimizer.step: expected a gradient of {self.n_params} elements")
        check(self.lib.nrs_optimizer_step(self.h, _stream_handle(stream), grad.data_ptr(), float(loss_scale), float(lr), 1 if zero_grad else 0))

    def step_count(self):
        return int(self.lib.nrs_optimizer_step_count(self.h))

    def set_step_count(self, steps):
        check(self.lib.nrs_optimizer_set_step_count(self.h, int(steps)))

    def get_state(self, which):
        """One state array as numpy (synchronous): _abi.OPT_MASTER / OPT_M / OPT_V / OPT_EMA float32, OPT_STEPS uint32, OPT_PARAMS_FP16 float16."""
        if which not in self._DTYPES:
            raise NrsError("Optimizer.get_state: unknown state array")
        out = np.empty(self.n_params, dtype=self._DTYPES[which])
        check(self.lib.nrs_optimizer_get_state(self.h, int(which), out.ctypes.data, out.size))
        return out

    def set_state(self, which, values):
        if which not in self._DTYPES:
            raise NrsError("Optimizer.set_state: unknown state array")
        v = np.ascontiguousarray(values)
        if v.dtype != self._DTYPES[which]:
            raise NrsError(f"Optimizer.set_state: expected dtype {np.dtype(self._DTYPES[which])}")
        check(self.lib.nrs_optimizer_set_state(self.h, int(which), v.ctypes.data, v.size))

    def export_fp16(self, which=_abi.OPT_EXPORT_WEIGHTS, out=None, stream=None):
        """The whole blob as an fp16 CUDA tensor: the weights the network reads, or the rounded EMA (what a second network renders with: set_params_device)."""
        if out is None:
            out = torch.empty(self.n_params, dtype=torch.float16, device=f"cuda:{self.ctx.device}")
        _require_cuda(out, torch.float16, "out")
        if out.numel() != self.n_params:
            raise NrsError(f"Optimizer.export_fp16: out must hold {self.n_params} elements")
        check(self.lib.nrs_optimizer_export_fp16(self.h, int(which), out.data_ptr(), _stream_handle(stream)))
        return out

    def close(self):
        if self.h:
            self.lib.nrs_optimizer_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def adam_bias_table(beta1=0.9, beta2=0.99):
    """nrs_adam_bias_table as numpy float32: entry t - 1 is bias(t) = sqrt(1 - beta2^t) / (1 - beta1^t), up to the t from which on it is 1.0f.  Host only."""
    lib = _abi.load()
    n = C.c_uint32()
    check(lib.nrs_adam_bias_table(float(beta1), float(beta2), None, 0, C.byref(n)))
    out = np.empty(n.value, dtype=np.float32)
    check(lib.nrs_adam_bias_table(float(beta1), float(beta2), out.ctypes.data, out.size, C.byref(n)))
    return out


def exponential_decay_lr(steps_done, base=_abi.BASE_LEARNING_RATE, decay_start=_abi.BASE_DECAY_START, decay_interval=_abi.BASE_DECAY_INTERVAL,
                         decay_base=_abi.BASE_DECAY_BASE):
    """nrs_exponential_decay_lr: the learning rate of the step that follows `steps_done` finished ones (base.json's schedule by default).  Host only."""
    return float(_abi.load().nrs_exponential_decay_lr(float(base), int(decay_start), int(decay_interval), float(decay_base), int(steps_done)))


class Dataset:
    """Posed images on the device (nrs_dataset_*): n_images images of one resolution as fp16 RGBA, linear and premultiplied (NerfDataset::images_data), and one camera
    record per image.  rays() is the first half of generate_training_samples_nerf: the pixels a training step looks at, their rays and the colours they should have."""

    _FORMATS = {np.dtype(np.uint8): (_abi.IMAGE_RGBA8_SRGB, torch.uint8), np.dtype(np.float32): (_abi.IMAGE_RGBA32F_LINEAR, torch.float32),
                np.dtype(np.float16): (_abi.IMAGE_RGBA16F_LINEAR, torch.float16)}

    def __init__(self, ctx, n_images, width, height):
        self.ctx, self.lib = ctx, ctx.lib
        self.n_images, self.width, self.height = int(n_images), int(width), int(height)
        self.h = C.c_void_p()
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
        dev = f"cuda:{self.ctx.device}"
        p = _abi.DatasetRaysParams()
        p.n_rays_total, p.rng_state, p.rng_inc = int(n_rays_total) & 0xffffffff, int(rng[0]), int(rng[1])
        p.snap_to_pixel_centers, p.random_bg_color = int(bool(snap)), int(bool(random_bg))
        rays = torch.empty((n, 6), dtype=torch.float32, device=dev)
        jitter = torch.empty(n, dtype=torch.float32, device=dev)
        target = torch.empty((n, 4), dtype=torch.float32, device=dev)
        background = torch.empty((n, 3), dtype=torch.float32, device=dev) if random_bg else None
        pixels = torch.empty((n, 2), dtype=torch.int32, device=dev) if want_pixels else None
        check(self.lib.nrs_dataset_rays(self.h, _stream_handle(stream), C.byref(p), n, rays.data_ptr(), jitter.data_ptr(), target.data_ptr(),
                                        None if background is None else background.data_ptr(), None if pixels is None else pixels.data_ptr()))
        return rays, jitter, target, background, pixels

    def mark_untrained(self, network, clear_visible=True, stream=None):
        """mark_untrained_density_grid on the network's density grid: cells no camera sees become -1 (and stay so through every later grid update), seen cells 0 where
        clear_visible or their sign disagrees; the bitfield is rebuilt.  Waits for the stream, like every bitfield rebuild."""
        check(self.lib.nrs_dataset_mark_untrained(network.h, self.h, 1 if clear_visible else 0, _stream_handle(stream)))

    def close(self):
        if self.h:
            self.lib.nrs_dataset_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def rng_advance(state, inc, delta=_abi.RNG_STEP_DELTA):
    """nrs_rng_advance: pcg32's state after `delta` more steps.  Host only."""
    st = C.c_uint64(int(state))
    _abi.load().nrs_rng_advance(C.byref(st), int(inc), int(delta) & 0xffffffffffffffff)
    return st.value


class CageDeformation:
    """One cage-deformation edit operator; owns its GPU tables (tet_mesh.h:80-94)."""

    def __init__(self, ctx, desc, cage_edit, device_authoring=False):
        self.ctx, self.lib = ctx, ctx.lib
        self.host = cage_edit  # keeps the numpy arrays alive
        self.h = C.c_void_p()
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

    def close(self):
        if self.h:
            self.lib.nrs_edit_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class AffineDuplication(CageDeformation):
    """AffineDuplication edit operator (editing/affine_duplication.h): shares map_rays / map_positions with the cage operator."""

    def __init__(self, ctx, desc, op):
        self.ctx, self.lib = ctx, ctx.lib
        self.host = op
        self.h = C.c_void_p()
        self.n_vertices = self.n_tets = 0
        check(self.lib.nrs_edit_create_affine(ctx.h, C.byref(desc), C.byref(op), C.byref(self.h)))


class RenderBuffer:
    """frame_buffer(): f32x4 premultiplied linear RGBA [H, W, 4]; depth_buffer(): f32 [H, W]; spp(): Sobol sample index."""

    def __init__(self, width, height, device="cuda:0", with_steps=False):
        self.width, self.height = int(width), int(height)
        self._frame = torch.zeros((self.height, self.width, 4), dtype=torch.float32, device=device)
        self._depth = torch.zeros((self.height, self.width), dtype=torch.float32, device=device)
        self._steps = torch.zeros((self.height, self.width), dtype=torch.int32, device=device) if with_steps else None
        self._spp = 0

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

    def accumulate(self, ctx, stream=None, color_space=0):
        """CudaRenderBuffer::accumulate (render_buffer.cu:540): the frame buffer joins the running mean of this view's spp frames; spp() counts them."""
        if getattr(self, "_accumulate", None) is None:
            self._accumulate = torch.zeros_like(self._frame)
        check(_abi.load().nrs_accumulate(ctx.h, _stream_handle(stream), self.width, self.height, self._frame.data_ptr(), self._accumulate.data_ptr(), int(self._spp), int(color_space)))
        self._spp += 1
        return self._accumulate

    def spp_slabs(self, spp_count):
        """Frame [K, H, W, 4], depth [K, H, W] and (with_steps) steps [K, H, W] slabs for Testbed.render_nerf_spp: allocated on first use, the frame slabs cleared on every call."""
        k = int(spp_count)
        if getattr(self, "_slabs", None) is None or self._slabs[0].shape[0] != k:
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
        _require_cuda(frames, torch.float32, "frames")
        if frames.dim() != 4 or tuple(frames.shape[1:]) != (self.height, self.width, 4):
            raise ValueError(f"frames must be [K, {self.height}, {self.width}, 4], got {tuple(frames.shape)}")
        if getattr(self, "_accumulate", None) is None:
            self._accumulate = torch.zeros_like(self._frame)
        k = int(frames.shape[0])
        check(_abi.load().nrs_accumulate_spp(ctx.h, _stream_handle(stream), self.width, self.height, frames.data_ptr(), self.width * self.height, k,
                                             self._accumulate.data_ptr(), int(self._spp), int(color_space)))
        self._spp += k
        return self._accumulate

    def set_color_space(self, color_space):
        """CudaRenderBuffer::set_color_space (render_buffer.h:233): the EColorSpace of the accumulate buffer, read by tonemap() and accumulate_spp_tonemap()."""
        if int(color_space) != getattr(self, "_color_space", 0):   # (a change resets the accumulation, as there)
            self._color_space = int(color_space)
            self._spp = 0

    def set_tonemap_curve(self, curve):
        """CudaRenderBuffer::set_tonemap_curve (render_buffer.h:233): ETonemapCurve, 0 Identity, 1 ACES, 2 Hable, 3 Reinhard."""
        if int(curve) != getattr(self, "_tonemap_curve", 0):
            self._tonemap_curve = int(curve)
            self._spp = 0

    _TONEMAP_FORMATS = {"rgba32f": _abi.TONEMAP_RGBA32F, "rgba8": _abi.TONEMAP_RGBA8}

    def _tonemap_params(self, exposure, background, output_color_space, fmt, clamp_output):
        if fmt not in self._TONEMAP_FORMATS:
            raise ValueError(f"fmt is 'rgba32f' or 'rgba8', got {fmt!r}")
        t = _abi.TonemapParams()
        t.exposure = float(exposure)
        t.background_color[:] = [float(v) for v in background]
        t.color_space = getattr(self, "_color_space", 0)
        t.output_color_space = int(output_color_space)
        t.tonemap_curve = getattr(self, "_tonemap_curve", 0)
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
        if getattr(self, "_accumulate", None) is None:
            raise NrsError("RenderBuffer.tonemap: nothing has been accumulated")
        t = self._tonemap_params(exposure, background, output_color_space, fmt, clamp_output)
        out = self._tonemap_output(fmt)
        check(_abi.load().nrs_tonemap(ctx.h, _stream_handle(stream), self.width, self.height, self._accumulate.data_ptr(), C.byref(t), out.data_ptr()))
        return out

    def accumulate_spp_tonemap(self, ctx, frames, exposure=0.0, background=(0.0, 0.0, 0.0, 0.0), output_color_space=1, fmt="rgba32f", stream=None, clamp_output=False):
        """accumulate_spp(ctx, frames, color_space of set_color_space) followed by tonemap(...), in one pass over the accumulate buffer (nrs_accumulate_spp_tonemap):
        bit-equal to the pair.  spp() advances by K; returns the output tensor as tonemap() does."""
        _require_cuda(frames, torch.float32, "frames")
        if frames.dim() != 4 or tuple(frames.shape[1:]) != (self.height, self.width, 4):
            raise ValueError(f"frames must be [K, {self.height}, {self.width}, 4], got {tuple(frames.shape)}")
        if getattr(self, "_accumulate", None) is None:
            self._accumulate = torch.zeros_like(self._frame)
        t = self._tonemap_params(exposure, background, output_color_space, fmt, clamp_output)
        out = self._tonemap_output(fmt)
        k = int(frames.shape[0])
        check(_abi.load().nrs_accumulate_spp_tonemap(ctx.h, _stream_handle(stream), self.width, self.height, frames.data_ptr(), self.width * self.height, k,
                                                     self._accumulate.data_ptr(), int(self._spp), C.byref(t), out.data_ptr()))
        self._spp += k
        return out

    def accumulate_buffer(self):
        return getattr(self, "_accumulate", None)

    def clear_frame(self, stream=None):
        self._frame.zero_()
        self._depth.zero_()


class Mesh:
    """nrs_mesh: a triangle mesh on the device (m_mesh's verts, vert_normals, vert_colors, verts_smoothed, indices)"""

    def __init__(self, lib, handle):
        self.lib, self.h = lib, handle
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
                                      C.byref((C.c_float * 3)(*offset))))

    def close(self):
        if self.h:
            self.lib.nrs_mesh_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def mesh_from_density(ctx, density, aabb_min, aabb_max, thresh, stream=None):
    """marching_cubes_gpu + compute_mesh_1ring on a caller's field: a float32 CUDA tensor [rz, ry, rx] (what Testbed.get_density_on_grid returns) -> Mesh"""
    _require_cuda(density, torch.float32, "density")
    if density.dim() != 3 or not density.is_contiguous():
        raise NrsError("mesh_from_density: density must be a contiguous [rz, ry, rx] tensor")
    rz, ry, rx = density.shape
    h = C.c_void_p()
    check(ctx.lib.nrs_mesh_from_density(ctx.h, _stream_handle(stream), C.byref((C.c_uint32 * 3)(rx, ry, rz)), C.byref((C.c_float * 3)(*aabb_min)),
                                        C.byref((C.c_float * 3)(*aabb_max)), float(thresh), density.data_ptr(), C.byref(h)))
    return Mesh(ctx.lib, h)


class GrowingSelection:
    """nrs_selection: RegionGrowing (region_growing.cu) with GrowingSelection's dilate / erode / extract_fine_mesh (growing_selection.cu:2083-2162).  Growing and the
    accessors are host-only; dilate, erode and extract_fine_mesh need a Context (ctx may be None until then)."""

    def __init__(self, ctx, density_grid, max_cascade=0, lib=None):
        self.ctx, self.lib = ctx, lib if lib is not None else (ctx.lib if ctx is not None else _abi.load())
        grid = np.ascontiguousarray(density_grid, np.float32).reshape(-1)
        self.h = C.c_void_p()
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

    def close(self):
        if self.h:
            self.lib.nrs_selection_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


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


def set_camera_extras(p, render_distortion=None, distortion_map=None, envmap=None):
    """Camera model and background of an nrs_render_params (init_rays_from_camera's arguments, testbed_nerf.cu:3078-3100): lens distortion (mode, 7 params),
    the distortion map [H, W, 2] and the environment map [H, W, 4] as float32 CUDA tensors (the struct keeps raw device pointers: keep the tensors alive)."""
    if render_distortion is not None:
        p.distortion_mode = int(render_distortion[0])
        p.distortion_params[:] = [float(v) for v in render_distortion[1]]
    if distortion_map is not None:
        _require_cuda(distortion_map, torch.float32, "distortion_map")
        p.d_distortion_map = distortion_map.data_ptr()
        p.distortion_resolution[:] = (distortion_map.shape[1], distortion_map.shape[0])
    if envmap is not None:
        _require_cuda(envmap, torch.float32, "envmap")
        p.d_envmap = envmap.data_ptr()
        p.envmap_resolution[:] = (envmap.shape[1], envmap.shape[0])
    return p


class Testbed:
    """The slice of ngp::Testbed the render path reads: network, occupancy, edit operators and the render knobs."""

    def __init__(self, ctx, desc, aabb_scale=1, n_extra_dims=0):
        self.ctx, self.lib, self.desc = ctx, ctx.lib, desc
        self.nerf_network = NerfNetwork(ctx, desc, n_extra_dims=n_extra_dims)
        self.edit_operators = []          # NerfTracer::m_edit_operators, applied last-to-first
        self.enable_edits = True          # m_enable_edits
        self.snap_to_pixel_centers = True
        self.rendering_min_transmittance = 0.01
        self.cone_angle_constant = 0.0 if aabb_scale <= 1 else 1.0 / 256.0
        self.render_mode = _abi.RENDER_SHADE
        self.linear_colors = False
        self.show_accel = -1              # m_nerf.show_accel
        self.dof = 0.0                    # m_dof
        self.slice_plane_z, self.scale = 0.0, 1.0   # m_slice_plane_z, m_scale
        self.dataset_scale = 1.0          # m_nerf.training.dataset.scale
        self.render_distortion = (0, (0.0,) * 7)   # m_nerf.render_distortion (mode, params) when render_with_camera_distortion
        self.distortion_map = None        # m_distortion.map: float32 CUDA tensor [H, W, 2] or None
        self.envmap = None                # m_envmap.envmap: float32 CUDA tensor [H, W, 4] or None
        self.glow_mode, self.glow_y_cutoff = 0, 0.0   # m_nerf.m_glow_mode / m_glow_y_cutoff
        mn, mx = list(desc.aabb_min), list(desc.aabb_max)
        self.render_aabb = (mn, mx)       # m_render_aabb
        self.last_stats = None
        self.m_camera = None              # m_camera: 3x4 column-major [12]; set by set_camera_from_time / render_to_cpu
        self.m_smoothed_camera = None     # m_smoothed_camera: the camera the last frame ended on
        self.camera_smoothing = False     # m_camera_smoothing
        self.fov, self.fov_axis = 50.625, 1   # fov() in degrees (set_camera_from_time sets it), m_fov_axis
        self.camera_path = []             # m_camera_path.m_keyframes: a list of _abi.CameraKeyframe

    def add_edit_operator(self, op):
        self.edit_operators.append(op)

    def training_samples(self, rays, jitter=None, max_samples=1 << 18, cone_angle_constant=None, stream=None):
        """The network inputs of a batch of training rays (NerfNetwork.training_samples) with this testbed's cone angle: coords, numsteps, ray_indices, counters."""
        cone = self.cone_angle_constant if cone_angle_constant is None else cone_angle_constant
        return self.nerf_network.training_samples(stream, rays, jitter, cone, max_samples)

    def make_params(self, render_buffer, focal_length, camera_matrix0, camera_matrix1, rolling_shutter, screen_center, apply_operators):
        p = RenderParams()
        p.resolution[:] = render_buffer.in_resolution()
        p.focal_length[:] = list(focal_length)
        p.camera_matrix0[:] = [float(v) for v in np.asarray(camera_matrix0, np.float32).reshape(-1)]
        p.camera_matrix1[:] = [float(v) for v in np.asarray(camera_matrix1, np.float32).reshape(-1)]
        p.rolling_shutter[:] = list(rolling_shutter)
        p.screen_center[:] = list(screen_center)
        p.render_aabb_min[:] = self.render_aabb[0]
        p.render_aabb_max[:] = self.render_aabb[1]
        p.spp_index = render_buffer.spp()
        p.snap_to_pixel_centers = 1 if self.snap_to_pixel_centers else 0
        p.min_transmittance = self.rendering_min_transmittance
        p.cone_angle_constant = self.cone_angle_constant
        p.render_mode = self.render_mode
        p.linear_colors = 1 if self.linear_colors else 0
        p.apply_operators = 1 if apply_operators else 0
        p.min_mip = self.show_accel if self.show_accel >= 0 else 0
        p.show_accel = 1 if self.show_accel >= 0 else 0
        p.dof = self.dof
        p.slice_plane_z = self.slice_plane_z + self.scale  # testbed_nerf.cu:3067
        p.depth_scale = 1.0 / self.dataset_scale           # :3113
        p.glow_mode, p.glow_y_cutoff = self.glow_mode, self.glow_y_cutoff
        set_camera_extras(p, self.render_distortion, self.distortion_map, self.envmap)
        return p

    def render_nerf(self, network, render_buffer, max_res, focal_length, camera_matrix0, camera_matrix1, rolling_shutter, screen_center,
                    apply_operators, stream=None, want_stats=False):
        """Testbed::render_nerf(network, render_buffer, max_res, focal_length, camera_matrix0, camera_matrix1, rolling_shutter,
        screen_center, apply_operators, stream).  The frame buffer must have been cleared by the caller (render_frame does)."""
        p = self.make_params(render_buffer, focal_length, camera_matrix0, camera_matrix1, rolling_shutter, screen_center,
                             apply_operators and self.enable_edits)
        return self.render_with_params(network, p, render_buffer.frame_buffer(), render_buffer.depth_buffer(), render_buffer.steps_buffer(),
                                       stream, want_stats)

    def render_with_params(self, network, p, frame, depth, steps=None, stream=None, want_stats=False):
        _require_cuda(frame, torch.float32, "frame_buffer")
        _require_cuda(depth, torch.float32, "depth_buffer")
        n = len(self.edit_operators)
        arr = (C.c_void_p * max(n, 1))(*[op.h for op in self.edit_operators])
        stats = RenderStats() if want_stats else None
        check(self.lib.nrs_render_nerf(network.h, C.byref(p), arr, n, frame.data_ptr(), depth.data_ptr(),
                                       steps.data_ptr() if steps is not None else None, _stream_handle(stream),
                                       C.byref(stats) if stats is not None else None))
        self.last_stats = stats
        return stats

    def render_nerf_spp(self, network, render_buffer, spp_count, focal_length, camera_matrix0, camera_matrix1, rolling_shutter, screen_center,
                        apply_operators, stream=None, want_stats=False):
        """Samples spp() .. spp() + spp_count - 1 of the view in ONE launch (what the spp loop of the reference's render_to_cpu does in spp_count launches): returns
        (frames [K, H, W, 4], depths [K, H, W], steps or None, stats).  Follow with render_buffer.accumulate_spp(ctx, frames), which advances spp() by K."""
        p = self.make_params(render_buffer, focal_length, camera_matrix0, camera_matrix1, rolling_shutter, screen_center,
                             apply_operators and self.enable_edits)
        frames, depths, steps = render_buffer.spp_slabs(spp_count)
        stats = self.render_spp_with_params(network, p, spp_count, frames, depths, steps, None, stream, want_stats)
        return frames, depths, steps, stats

    def render_spp_with_params(self, network, p, spp_count, frames, depths, steps=None, slab_stride_pixels=None, stream=None, want_stats=False):
        """nrs_render_nerf_spp: slab k of frames / depths / steps (slab_stride_pixels apart; default: the elements of frames[0] / 4) receives sample p.spp_index + k."""
        _require_cuda(frames, torch.float32, "frames")
        _require_cuda(depths, torch.float32, "depths")
        if slab_stride_pixels is None:
            slab_stride_pixels = frames[0].numel() // 4 if frames.dim() > 1 and frames.shape[0] else 0
        n = len(self.edit_operators)
        arr = (C.c_void_p * max(n, 1))(*[op.h for op in self.edit_operators])
        stats = RenderStats() if want_stats else None
        check(self.lib.nrs_render_nerf_spp(network.h, C.byref(p), arr, n, int(spp_count), frames.data_ptr(), depths.data_ptr(),
                                           steps.data_ptr() if steps is not None else None, int(slab_stride_pixels), _stream_handle(stream),
                                           C.byref(stats) if stats is not None else None))
        self.last_stats = stats
        return stats

    def render_spp_with_views(self, network, p, views, frames, depths, steps=None, slab_stride_pixels=None, stream=None, want_stats=False, spp_count=None):
        """nrs_render_nerf_spp_views: slab k receives sample p.spp_index + k rendered with views[k] (a ctypes array of _abi.SampleView, or a list of them) in place of
        p's cameras, focal length, dof and slice_plane_z.  One launch for the whole batch.  views = None is nrs_render_nerf_spp of `spp_count` samples; spp_count
        defaults to len(views)."""
        _require_cuda(frames, torch.float32, "frames")
        _require_cuda(depths, torch.float32, "depths")
        if views is not None and not isinstance(views, C.Array):
            views = (_abi.SampleView * max(len(views), 1))(*views)
        if spp_count is None:
            spp_count = len(views)
        if slab_stride_pixels is None:
            slab_stride_pixels = frames[0].numel() // 4 if frames.dim() > 1 and frames.shape[0] else 0
        n = len(self.edit_operators)
        arr = (C.c_void_p * max(n, 1))(*[op.h for op in self.edit_operators])
        stats = RenderStats() if want_stats else None
        check(self.lib.nrs_render_nerf_spp_views(network.h, C.byref(p), arr, n, int(spp_count), C.cast(views, C.c_void_p) if views is not None else None, frames.data_ptr(), depths.data_ptr(),
                                                 steps.data_ptr() if steps is not None else None, int(slab_stride_pixels), _stream_handle(stream),
                                                 C.byref(stats) if stats is not None else None))
        self.last_stats = stats
        return stats

    # ---- the camera path (CameraPath, Testbed::set_camera_from_time / apply_camera_smoothing) ----
    def load_camera_path(self, path):
        """Testbed::load_camera_path -> CameraPath::load (src/camera_path.cu:114-136): the keyframes of a file CameraPath::save wrote; returns their number"""
        h = C.c_void_p()
        check(self.lib.nrs_camera_path_open(os.fsencode(path), C.byref(h)))
        try:
            n = self.lib.nrs_camera_path_count(h)
            keys = (_abi.CameraKeyframe * max(n, 1))()
            check(self.lib.nrs_camera_path_keyframes(h, C.cast(keys, C.c_void_p), n))
        finally:
            self.lib.nrs_camera_path_close(h)
        self.camera_path = [keys[i] for i in range(n)]
        return n

    def _path_array(self):
        n = len(self.camera_path)
        return (_abi.CameraKeyframe * max(n, 1))(*self.camera_path), n

    def set_camera_from_time(self, t):
        """Testbed::set_camera_from_time (src/testbed.cu:2099-2111): m_camera, slice / scale, fov and dof from the path's keyframe at t; nothing without a path"""
        keys, n = self._path_array()
        if n == 0:
            return
        k = _abi.CameraKeyframe()
        check(self.lib.nrs_camera_path_eval(C.cast(keys, C.c_void_p), n, float(t), C.byref(k)))
        m = (C.c_float * 12)()
        check(self.lib.nrs_camera_keyframe_matrix(C.byref(k), C.byref(m)))
        self.m_camera = list(m)
        self.slice_plane_z, self.scale, self.fov, self.dof = k.slice, k.scale, k.fov, k.dof

    def log_space_lerp(self, begin, end, t):
        a, b, out = (C.c_float * 12)(*[float(v) for v in begin]), (C.c_float * 12)(*[float(v) for v in end]), (C.c_float * 12)()
        check(self.lib.nrs_log_space_lerp(C.byref(a), C.byref(b), float(t), C.byref(out)))
        return list(out)

    def apply_camera_smoothing(self, elapsed_ms):
        """Testbed::apply_camera_smoothing (src/testbed.cu:2086-2093)"""
        if self.camera_smoothing and self.m_smoothed_camera is not None:
            decay = float(np.float32(0.02) ** np.float32(elapsed_ms / 1000.0))
            self.m_smoothed_camera = self.log_space_lerp(self.m_smoothed_camera, self.m_camera, float(np.float32(1.0) - np.float32(decay)))
        else:
            self.m_smoothed_camera = list(self.m_camera)

    def motion_views(self, start, end, shutter_fraction, spp_count, first_sample, spp_total, resolution, start_time, end_time, base_view):
        """nrs_motion_views over this testbed's camera path -> a ctypes array of spp_count _abi.SampleView"""
        keys, n = self._path_array()
        a, b = (C.c_float * 12)(*[float(v) for v in start]), (C.c_float * 12)(*[float(v) for v in end])
        res = (C.c_int32 * 2)(int(resolution[0]), int(resolution[1]))
        out = (_abi.SampleView * int(spp_count))()
        check(self.lib.nrs_motion_views(C.byref(a), C.byref(b), float(shutter_fraction), int(spp_count), int(first_sample), int(spp_total), C.byref(res), int(self.fov_axis),
                                        C.cast(keys, C.c_void_p) if n else None, n, float(start_time), float(end_time), C.byref(base_view), C.cast(out, C.c_void_p)))
        return out

    def render_to_cpu(self, network, width, height, spp, linear, focal_length, camera_matrix0, camera_matrix1=None, rolling_shutter=(0.0, 0.0, 0.0, 0.0),
                      screen_center=(0.5, 0.5), exposure=0.0, background=(0.0, 0.0, 0.0, 0.0), fmt="rgba32f", tonemap_curve=0, color_space=0, apply_operators=True,
                      stream=None, start_time=-1.0, end_time=-1.0, fps=30.0, shutter_fraction=1.0, motion_blur=None):
        """Testbed::render_to_cpu(width, height, spp, linear, start_time, end_time, fps, shutter_fraction) (src/python_api.cu:129-175): the accumulation is reset, `spp`
        samples are rendered in batches of at most NRS_SPP_BATCH_MAX (one launch each) and folded into the running mean, and the last fold is fused with the display
        step (tonemap: `background`, `exposure`, `tonemap_curve`; sRGB output unless `linear`).  Returns a host array [H, W, 4]: float32 for fmt "rgba32f", uint8 for
        "rgba8".  The accumulate buffer stays readable as render_to_cpu_buffer().accumulate_buffer().

        A moving camera: with start_time >= 0 (the reference's own condition, python_api.cu:139) the frame runs from m_smoothed_camera to the (smoothed) camera of
        end_time -- the path's keyframe there, or without keyframes camera_matrix1 (camera_matrix0 when that is None) -- and over a path every sample takes fov, dof and
        focus plane from it at its own time.  Sample i renders between log_space_lerp(start, end, i / spp * shutter_fraction) and (i + 1) / spp * shutter_fraction
        (nrs_motion_views), a view per sample in one launch per batch, and m_smoothed_camera is left at the end camera.

        WHAT camera_matrix1 MEANS with start_time < 0 is decided by `motion_blur`.  False: the still call -- camera_matrix0 / camera_matrix1 go to every sample as they
        are (the two cameras of a rolling shutter) and shutter_fraction is not looked at.  True: camera_matrix1 is the end-of-shutter camera of a frame that starts at
        camera_matrix0, for every shutter_fraction, 1.0 included.  None (the default) is True exactly when shutter_fraction != 1.0: the reference's default shutter
        keeps the call what it was before these arguments existed, bit for bit -- so a full-shutter blur between two cameras has to be asked for with motion_blur=True."""
        spp = int(spp)
        if spp < 1:
            raise ValueError("spp must be at least 1")
        on_path = start_time >= 0.0
        if on_path or (float(shutter_fraction) != 1.0 if motion_blur is None else bool(motion_blur)):
            return self._render_to_cpu_moving(network, width, height, spp, linear, focal_length, camera_matrix0, camera_matrix1, rolling_shutter, screen_center, exposure,
                                              background, fmt, tonemap_curve, color_space, apply_operators, stream, start_time, end_time, fps, shutter_fraction, on_path)
        buf = getattr(self, "_windowless", None)
        if buf is None or buf.in_resolution() != (int(width), int(height)):
            buf = self._windowless = RenderBuffer(width, height, device=f"cuda:{self.ctx.device}")   # m_windowless_render_surface.resize
        buf.set_spp(0)                                                                                # reset_accumulation
        buf.set_color_space(color_space)
        buf.set_tonemap_curve(tonemap_curve)
        cam1 = camera_matrix0 if camera_matrix1 is None else camera_matrix1
        done, out = 0, None
        while done < spp:
            k = min(spp - done, _abi.SPP_BATCH_MAX)
            frames = self.render_nerf_spp(network, buf, k, focal_length, camera_matrix0, cam1, rolling_shutter, screen_center, apply_operators, stream)[0]
            if done + k < spp:
                buf.accumulate_spp(self.ctx, frames, stream, color_space)
            else:
                out = buf.accumulate_spp_tonemap(self.ctx, frames, exposure, background, 0 if linear else 1, fmt, stream)
            done += k
        if stream is not None:
            (stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(int(stream))).synchronize()
        return out.cpu().numpy()

    def _render_to_cpu_moving(self, network, width, height, spp, linear, focal_length, camera_matrix0, camera_matrix1, rolling_shutter, screen_center, exposure,
                              background, fmt, tonemap_curve, color_space, apply_operators, stream, start_time, end_time, fps, shutter_fraction, on_path):
        buf = getattr(self, "_windowless", None)
        if buf is None or buf.in_resolution() != (int(width), int(height)):
            buf = self._windowless = RenderBuffer(width, height, device=f"cuda:{self.ctx.device}")
        buf.set_spp(0)
        buf.set_color_space(color_space)
        buf.set_tonemap_curve(tonemap_curve)
        cam0 = [float(v) for v in np.asarray(camera_matrix0, np.float32).reshape(-1)]
        if on_path:                                                    # python_api.cu:133-146
            if end_time < 0.0:
                end_time = start_time
            start_cam = list(self.m_smoothed_camera) if self.m_smoothed_camera is not None else cam0
            if self.m_smoothed_camera is None:
                self.m_smoothed_camera = list(start_cam)
            if not self.camera_path:   # set_camera_from_time leaves m_camera alone without keyframes: the caller's camera is the current one
                self.m_camera = cam0 if camera_matrix1 is None else [float(v) for v in np.asarray(camera_matrix1, np.float32).reshape(-1)]
            self.set_camera_from_time(end_time)
            self.apply_camera_smoothing(1000.0 / fps)
            end_cam = list(self.m_smoothed_camera)
        else:
            start_cam = cam0
            end_cam = cam0 if camera_matrix1 is None else [float(v) for v in np.asarray(camera_matrix1, np.float32).reshape(-1)]
            self.m_camera = list(end_cam)
            start_time = -1.0
        base = _abi.SampleView()
        base.focal_length[:] = list(focal_length)
        base.dof, base.slice_plane_z = self.dof, self.slice_plane_z + self.scale
        done, out = 0, None
        while done < spp:
            k = min(spp - done, _abi.SPP_BATCH_MAX)
            views = self.motion_views(start_cam, end_cam, shutter_fraction, k, done, spp, (width, height), start_time, end_time, base)
            p = self.make_params(buf, focal_length, views[0].camera_matrix0, views[0].camera_matrix1, rolling_shutter, screen_center, apply_operators and self.enable_edits)
            frames, depths, steps = buf.spp_slabs(k)
            self.render_spp_with_views(network, p, views, frames, depths, steps, None, stream)
            if done + k < spp:
                buf.accumulate_spp(self.ctx, frames, stream, color_space)
            else:
                out = buf.accumulate_spp_tonemap(self.ctx, frames, exposure, background, 0 if linear else 1, fmt, stream)
            done += k
        if on_path:   # the loop's last set_camera_from_time: the testbed is left on the last sample's keyframe
            a0 = np.float32(spp - 1) / np.float32(spp) * np.float32(shutter_fraction)
            a1 = (np.float32(spp - 1) + np.float32(1.0)) / np.float32(spp) * np.float32(shutter_fraction)
            self.set_camera_from_time(float(np.float32(start_time) + (np.float32(end_time) - np.float32(start_time)) * (a0 + a1) / np.float32(2.0)))
        self.m_smoothed_camera = list(end_cam)                         # python_api.cu:167-168
        if stream is not None:
            (stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(int(stream))).synchronize()
        return out.cpu().numpy()

    def render_to_cpu_buffer(self):
        """The RenderBuffer render_to_cpu renders into (m_windowless_render_surface); None before the first call."""
        return getattr(self, "_windowless", None)

    def get_density_on_grid(self, res3d, aabb_min, aabb_max, mask_with_density_grid=True, stream=None):
        """Testbed::get_density_on_grid(res3d, aabb) (testbed_nerf.cu:4538) -> float32 CUDA tensor [rz, ry, rx]"""
        res = (C.c_uint32 * 3)(*[int(v) for v in res3d])
        mn, mx = (C.c_float * 3)(*aabb_min), (C.c_float * 3)(*aabb_max)
        out = torch.zeros((int(res3d[2]), int(res3d[1]), int(res3d[0])), dtype=torch.float32, device=f"cuda:{self.ctx.device}")
        check(self.lib.nrs_density_on_grid(self.nerf_network.h, _stream_handle(stream), C.byref(res), C.byref(mn), C.byref(mx),
                                           1 if mask_with_density_grid else 0, out.data_ptr()))
        return out

    # ---- mesh extraction (Testbed::marching_cubes and its Python callers) ----
    @staticmethod
    def get_marching_cubes_res(res_1d, aabb_min, aabb_max):
        """get_marching_cubes_res(res_1d, aabb) (marching_cubes.cu:48) -> (rx, ry, rz), each a multiple of 16; host-only"""
        out = (C.c_uint32 * 3)()
        check(_abi.load().nrs_marching_cubes_res(int(res_1d), C.byref((C.c_float * 3)(*aabb_min)), C.byref((C.c_float * 3)(*aabb_max)), C.byref(out)))
        return tuple(out)

    def _mesh_aabb(self, aabb):
        if aabb is None or len(aabb) == 0:   # aabb.is_empty(): the render box (python_api.cu:106-108)
            return self.render_aabb
        return aabb

    def marching_cubes(self, res3d, aabb=None, thresh=_abi.MESH_THRESH_DEFAULT, mask_with_density_grid=True, stream=None):
        """Testbed::marching_cubes(res3d, aabb, thresh) (testbed_nerf.cu:4614): the mesh stays on the testbed (self.mesh, m_mesh); returns the number of triangles."""
        if np.isscalar(res3d):
            res3d = (res3d,) * 3
        mn, mx = self._mesh_aabb(aabb)
        h = C.c_void_p()
        check(self.lib.nrs_mesh_extract(self.nerf_network.h, _stream_handle(stream), C.byref((C.c_uint32 * 3)(*[int(v) for v in res3d])), C.byref((C.c_float * 3)(*mn)),
                                        C.byref((C.c_float * 3)(*mx)), float(thresh), 1 if mask_with_density_grid else 0, 1 if self.linear_colors else 0, C.byref(h)))
        if getattr(self, "mesh", None) is not None:
            self.mesh.close()
        self.mesh = Mesh(self.lib, h)
        return self.mesh.n_tris

    def compute_marching_cubes_mesh(self, res3d=128, aabb=None, thresh=_abi.MESH_THRESH_DEFAULT):
        """Testbed::compute_marching_cubes_mesh (python_api.cu:105-127) -> {"V", "N", "C": float32 [n_verts_padded, 3], "F": int32 [n_tris, 3]}; N normalised on the host"""
        self.marching_cubes(res3d, aabb, thresh)
        V, N, Cc, _, F = self.mesh.download()
        with np.errstate(invalid="ignore", divide="ignore"):
            sq = (N * N).sum(axis=1, dtype=np.float32)
            N = np.where(sq[:, None] > 0, N / np.sqrt(sq, dtype=np.float32)[:, None], N).astype(np.float32)   # Eigen's normalize(): a zero vector stays
        return {"V": V, "N": N, "C": Cc, "F": F.view(np.int32)}

    def compute_and_save_marching_cubes_mesh(self, filename, res3d=128, aabb=None, thresh=_abi.MESH_THRESH_DEFAULT, unwrap_it=False, dataset_offset=(0.0, 0.0, 0.0)):
        """Testbed::compute_and_save_marching_cubes_mesh (testbed.cu:337-343): positions go out as (v - dataset offset) / dataset scale; .ply is a PLY, anything else an OBJ"""
        if unwrap_it:
            raise NrsError("compute_and_save_marching_cubes_mesh: unwrap_it (the UV unwrap and its texture) is not built")
        self.marching_cubes(res3d, aabb, thresh)
        self.mesh.save(filename, self.dataset_scale, dataset_offset)

    def growing_selection(self, max_cascade=0):
        """A GrowingSelection over the model's density grid (m_density_grid copied to the host, as reset_growing does); max_cascade: m_max_cascade"""
        return GrowingSelection(self.ctx, self.nerf_network.get_density_grid(), max_cascade)

    def project_selection_pixels(self, params, pixels_xy, transmittance_threshold=0.1, automatic_max_level=True, growing_level=0, stream=None):
        """GrowingSelection::project_selection_pixels (growing_selection.cu:1832): scribbled pixels -> surface points and the
        occupancy cells they fall into.  Returns (positions [n, 3], cells [n], found [n]) per pixel plus the de-duplicated
        (cells, positions, growing_level) the region growing starts from."""
        px = torch.as_tensor(np.ascontiguousarray(pixels_xy, np.int32).reshape(-1, 2), device=f"cuda:{self.ctx.device}")
        n = px.shape[0]
        pos = torch.zeros((n, 3), dtype=torch.float32, device=px.device)
        cells = torch.zeros((n,), dtype=torch.int32, device=px.device)
        found = torch.zeros((n,), dtype=torch.uint8, device=px.device)
        check(self.lib.nrs_project_selection_pixels(self.nerf_network.h, _stream_handle(stream), C.byref(params), px.data_ptr(), n,
                                                    float(transmittance_threshold), pos.data_ptr(), cells.data_ptr(), found.data_ptr()))
        if stream is not None:
            stream.synchronize()
        else:
            torch.cuda.synchronize()
        h_pos, h_cells, h_found = pos.cpu().numpy(), cells.cpu().numpy().view(np.uint32), found.cpu().numpy()
        level = C.c_uint32(int(growing_level))
        out_cells, out_pos, n_out = np.zeros(n, np.uint32), np.zeros((n, 3), np.float32), C.c_uint32()
        check(self.lib.nrs_selection_cells(h_pos.ctypes.data, h_cells.ctypes.data, h_found.ctypes.data, n, 1 if automatic_max_level else 0,
                                           C.byref(level), out_cells.ctypes.data, out_pos.ctypes.data, C.byref(n_out)))
        return (h_pos, h_cells, h_found), (out_cells[: n_out.value], out_pos[: n_out.value], level.value)

    def compute_poisson_boundary(self, vertices, is_inside, jitter, sh_sampling_width=10, hemisphere_width=10):
        """GrowingSelection::compute_poisson_boundary (growing_selection.cu:2220): per cage vertex the density and the SH9 fit of
        the colours around it.  jitter: [n_verts * w * w, 2] in [0, 1] (the reference's std::rand() draws).  -> (density [n], sh [n, 27])"""
        v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
        jt = np.ascontiguousarray(jitter, np.float32)
        n = v.shape[0]
        if jt.size != n * sh_sampling_width * sh_sampling_width * 2:
            raise NrsError("compute_poisson_boundary: jitter must hold two draws per sample")
        density, sh = np.zeros(n, np.float32), np.zeros((n, 27), np.float32)
        check(self.lib.nrs_poisson_boundary(self.nerf_network.h, v.ctypes.data, n, int(sh_sampling_width), int(hemisphere_width), jt.ctypes.data,
                                            1 if is_inside else 0, density.ctypes.data, sh.ctypes.data))
        return density, sh

    def get_rgba_on_grid(self, res3d, ray_dir, stream=None):
        """Testbed::get_rgba_on_grid(res3d, ray_dir) (testbed_nerf.cu:4588) over m_render_aabb -> float32 CUDA tensor [rz, ry, rx, 4]"""
        res = (C.c_uint32 * 3)(*[int(v) for v in res3d])
        mn, mx, rd = (C.c_float * 3)(*self.render_aabb[0]), (C.c_float * 3)(*self.render_aabb[1]), (C.c_float * 3)(*ray_dir)
        out = torch.zeros((int(res3d[2]), int(res3d[1]), int(res3d[0]), 4), dtype=torch.float32, device=f"cuda:{self.ctx.device}")
        check(self.lib.nrs_rgba_on_grid(self.nerf_network.h, _stream_handle(stream), C.byref(res), C.byref(mn), C.byref(mx), C.byref(rd), out.data_ptr()))
        return out

    def new_grid_update(self, max_cascade=0, seed=1337, decay=0.95):
        """The Testbed members update_density_grid_nerf_operator reads: m_rng = default_rng_t{m_seed} (testbed.cu:2220),
        density_grid_ema_step = 0, density_grid_decay = 0.95 (testbed.h:604), sized as update_density_grid_nerf_render does."""
        u = _abi.GridUpdate()
        u.n_uniform_samples = _abi.GRID_VOLUME * (max_cascade + 1)
        u.n_nonuniform_samples = 0
        u.reset_grid = 0
        u.max_cascade = max_cascade
        u.decay = decay
        u.ema_step = 0
        st, inc = C.c_uint64(), C.c_uint64()
        self.lib.nrs_rng_seed(seed, C.byref(st), C.byref(inc))
        u.rng_state, u.rng_inc = st.value, inc.value
        return u

    def update_density_grid_nerf_operator(self, update, stream=None, apply_operators=True):
        """Testbed::update_density_grid_nerf_operator (testbed_nerf.cu:3533): one refresh of the occupancy in deformed space."""
        ops = self.edit_operators if (apply_operators and self.enable_edits) else []
        arr = (C.c_void_p * max(len(ops), 1))(*[op.h for op in ops])
        check(self.lib.nrs_model_update_density_grid(self.nerf_network.h, arr, len(ops), C.byref(update), _stream_handle(stream)))

    def update_density_grid_nerf_render(self, n_iterations, reset_grid, update, stream=None):
        """Testbed::update_density_grid_nerf_render (testbed_nerf.cu:3514)."""
        for i in range(n_iterations):
            update.reset_grid = 1 if (reset_grid and i == 0) else 0
            self.update_density_grid_nerf_operator(update, stream)
        update.reset_grid = 0

    def trace_samples(self, p, pixel_idx, max_samples, stream=None):
        """Test hook: (t, dt) stream per listed pixel -> (t [n, max], dt [n, max], count [n]) as CUDA tensors."""
        _require_cuda(pixel_idx, torch.int32, "pixel_idx")
        n = pixel_idx.numel()
        dev = pixel_idx.device
        t = torch.zeros((n, max_samples), dtype=torch.float32, device=dev)
        dt = torch.zeros((n, max_samples), dtype=torch.float32, device=dev)
        cnt = torch.zeros(n, dtype=torch.int32, device=dev)
        check(self.lib.nrs_trace_samples(self.nerf_network.h, C.byref(p), _stream_handle(stream), n, pixel_idx.data_ptr(), max_samples,
                                         t.data_ptr(), dt.data_ptr(), cnt.data_ptr()))
        return t, dt, cnt
