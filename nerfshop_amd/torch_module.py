"""NerfNetwork as a trainable torch module: one fp32 parameter tensor in the blob's order (density | rgb | grid), forward and backward on the HIP kernels.

The forward pass casts the parameters to fp16, hands them to the network on the device (nrs_model_set_params_device) and runs inference_mixed_precision; the
backward pass multiplies dL/doutput by the loss scale before the fp16 cast, runs nrs_network_backward and divides the fp32 parameter gradient by the scale.
`torch.optim` does the rest:

    net = NerfNetworkModule(seed=11)
    opt = torch.optim.Adam(net.parameters(), lr=1e-2, eps=1e-15)
    loss = ((net(coords)[:, :4] - target) ** 2).mean(); loss.backward(); opt.step()

Supported: base.json's architecture (nrs_network_backward).  The gradient with respect to the input reaches the position (floats 0..2 of a record) through the
hash grid only; the direction's gradient through the SH encoding is not propagated.  No second-order gradients.
"""
import math

import numpy as np
import torch

from . import runtime, synth
from ._abi import NrsError

LOSS_SCALE = 128.0  # tiny-cuda-nn's default for fp16 networks

# (n_out, n_in) of the five matrices in the blob's order: density network, rgb network (outputs padded to 16 rows)
MATRIX_SHAPES = ((64, 32), (16, 64), (64, 32), (64, 64), (16, 64))
N_MLP_PARAMS = sum(o * i for o, i in MATRIX_SHAPES)


def initial_params(n_params, seed):
    """tiny-cuda-nn's initialisation as recalled: Xavier-uniform matrices, U(-1e-4, 1e-4) hash-grid entries.  fp32 [n_params], on the CPU, a function of the seed."""
    gen = torch.Generator().manual_seed(int(seed))
    parts = []
    for n_out, n_in in MATRIX_SHAPES:
        limit = math.sqrt(6.0 / (n_in + n_out))
        parts.append((torch.rand(n_out * n_in, generator=gen) * 2.0 - 1.0) * limit)
    parts.append((torch.rand(n_params - N_MLP_PARAMS, generator=gen) * 2.0 - 1.0) * 1e-4)
    return torch.cat(parts).to(torch.float32)


class _NerfNetworkFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, params, coords, module):
        net = module.network
        p16 = params.detach().to(torch.float16)
        net.set_params_device(p16)
        module._resident = p16  # the blob the network holds now (and a reference until the stream has passed the copy)
        out = torch.empty((coords.shape[0], 16), dtype=torch.float16, device=coords.device)
        net.inference_mixed_precision(None, coords, out)
        ctx.module, ctx.p16 = module, p16
        ctx.save_for_backward(coords)
        return out.to(torch.float32)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        module, net = ctx.module, ctx.module.network
        coords, = ctx.saved_tensors
        if module._resident is not ctx.p16:  # another forward pass has replaced the parameters since
            net.set_params_device(ctx.p16)
            module._resident = ctx.p16
        dl = (grad_out * module.loss_scale).to(torch.float16).contiguous()
        grad_params = torch.empty(module.params.numel(), dtype=torch.float32, device=coords.device)
        grad_coords = torch.empty_like(coords) if ctx.needs_input_grad[1] else None
        net.backward(None, coords, dl, grad_params, grad_coords, accumulate=False)
        grad_params /= module.loss_scale
        if grad_coords is not None:
            grad_coords /= module.loss_scale
        return (grad_params if ctx.needs_input_grad[0] else None), grad_coords, None


class _RayLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, outputs, coords, numsteps, target_rgba, network, params, background, ray_origins, ray_counter):
        out16 = outputs.detach().to(torch.float16).contiguous()
        numsteps_out, _, dl, loss, _ = network.ray_loss(None, params, numsteps, coords, out16, target_rgba, background=background, ray_origins=ray_origins,
                                                        ray_counter=ray_counter)
        ctx.save_for_backward(numsteps, numsteps_out, dl, ray_counter if ray_counter is not None else torch.empty(0, device=outputs.device))
        ctx.loss_scale, ctx.shape = float(params.loss_scale), tuple(outputs.shape)
        return loss.sum()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        numsteps, numsteps_out, dl, ray_counter = ctx.saved_tensors
        n_rays, cap, dev = numsteps.shape[0], dl.shape[0], dl.device
        grad = torch.zeros(ctx.shape, dtype=torch.float32, device=dev)
        if n_rays == 0 or ctx.shape[0] == 0:
            return grad, None, None, None, None, None, None, None, None
        # The kernel wrote sample j < M' of ray r at compact index cbase_r + j; the output it belongs to is row base_r + j.  Found with a search over the rays' compact
        # ends instead of a read-back: rays at or past the counter have no samples.
        ray = torch.arange(n_rays, device=dev)
        live = ray < (ray_counter[0] if ray_counter.numel() else n_rays)
        cbase = numsteps_out[:, 1].to(torch.int64)
        ends = torch.where(live, cbase + numsteps_out[:, 0].to(torch.int64), torch.full_like(cbase, 1 << 40))
        k = torch.arange(cap, device=dev)
        r = torch.searchsorted(ends, k, right=True).clamp_(max=n_rays - 1)
        valid = live[r] & (k >= cbase[r]) & (k < ends[r])
        src = (numsteps[:, 1].to(torch.int64)[r] + (k - cbase[r])).clamp_(0, ctx.shape[0] - 1)
        vals = torch.where(valid[:, None], dl[:, :4].to(torch.float32), torch.zeros((), device=dev)) * (grad_loss / ctx.loss_scale)
        grad[:, :4].index_add_(0, src, vals)  # one non-zero term per row at most: the sum does not depend on the order
        return grad, None, None, None, None, None, None, None, None


def ray_loss(outputs, coords, numsteps, target_rgba, network, params, background=None, ray_origins=None, ray_counter=None):
    """The mean ray loss of compute_loss_kernel_train_nerf as a differentiable scalar.  outputs [n, 16] f32 (what NerfNetworkModule.forward returns for `coords`),
    coords [n, >= 7] f32, numsteps [n_rays, 2] int32 (count, base), target_rgba [n_rays, 4] f32; network: the runtime.NerfNetwork whose activations and box apply
    (module.network); params: RayLossParams with max_samples_compacted set.  The backward pass returns the kernel's dL/doutput divided by params.loss_scale: the derivative of
    the returned value with respect to `outputs` (plus the reference's regularisation terms, which have no loss behind them).  Early stops are decided on values."""
    if outputs.dim() != 2 or outputs.shape[1] != 16 or outputs.shape[0] != coords.shape[0]:
        raise NrsError("ray_loss: outputs must be [n, 16] with one row per coords record")
    return _RayLossFunction.apply(outputs, coords.contiguous(), numsteps, target_rgba, network, params, background, ray_origins, ray_counter)


class NerfNetworkModule(torch.nn.Module):
    """input [n, 7] f32 (warped position, dt, warped direction) -> [n, 16] f32: rgb raw, density raw, the rgb network's padding outputs."""

    def __init__(self, desc=None, params_fp16=None, seed=1337, ctx=None, device=0, loss_scale=LOSS_SCALE):
        super().__init__()
        self.desc = desc if desc is not None else synth.model_desc(1)
        self.ctx = ctx if ctx is not None else runtime.Context(device)
        # no cell-record cache: it would be rebuilt after every optimiser step
        self.network = runtime.NerfNetwork(self.ctx, self.desc, cell_cache_bytes=0)
        n_params = self.network.n_params()
        if params_fp16 is not None:
            blob = np.ascontiguousarray(params_fp16)
            if blob.dtype == np.uint16:
                blob = blob.view(np.float16)
            if blob.dtype != np.float16 or blob.size != n_params:
                raise NrsError(f"NerfNetworkModule: params_fp16 must hold {n_params} fp16 values")
            init = torch.from_numpy(blob.astype(np.float32))
        else:
            init = initial_params(n_params, seed)
        self.params = torch.nn.Parameter(init.to(f"cuda:{self.ctx.device}"))
        self.loss_scale = float(loss_scale)
        self._resident = None
        self._ray_bufs = None  # ray_step's device buffers, kept while the shapes stay

    def forward(self, coords):
        if coords.dim() != 2 or coords.shape[1] != 7:
            raise NrsError("NerfNetworkModule: input must be [n, 7]")
        return _NerfNetworkFunction.apply(self.params, coords.contiguous(), self)

    def ray_step(self, coords, numsteps, target_rgba, params, background=None, ray_origins=None, ray_counter=None):
        """One fused training step up to the optimiser: parameters to fp16, inference, nrs_ray_loss, nrs_network_backward on n = params.max_samples_compacted, then
        self.params.grad (+)= dL/dparams / params.loss_scale.  Returns the mean loss (a 0-d tensor on the device).  The outputs and dL/doutput stay fp16 on the device and
        nothing is read back; the caller runs optimizer.step().  coords [n, 7] f32, numsteps [n_rays, 2] int32, target_rgba [n_rays, 4] f32 as for ray_loss."""
        net = self.network
        coords = coords.contiguous()
        p16 = self.params.detach().to(torch.float16)
        net.set_params_device(p16)
        self._resident = p16
        key = (coords.shape[0], numsteps.shape[0], int(params.max_samples_compacted), coords.shape[1])
        if self._ray_bufs is None or self._ray_bufs[0] != key:
            dev = coords.device
            self._ray_bufs = (key, torch.empty((coords.shape[0], 16), dtype=torch.float16, device=dev),
                              net.ray_loss_buffers(numsteps.shape[0], params.max_samples_compacted, coords.shape[1], device=dev),
                              torch.empty(self.params.numel(), dtype=torch.float32, device=dev))
        _, out16, bufs, grad = self._ray_bufs
        net.inference_strided(None, coords, out16)
        _, coords_out, dl, loss, _ = net.ray_loss(None, params, numsteps, coords, out16, target_rgba, background=background, ray_origins=ray_origins,
                                                  ray_counter=ray_counter, out=bufs)
        net.backward(None, coords_out, dl, grad, None, accumulate=False)
        if self.params.grad is None:  # (once, or after every zero_grad(set_to_none=True): with set_to_none=False a step allocates nothing)
            self.params.grad = torch.zeros_like(self.params)
        self.params.grad.add_(grad, alpha=1.0 / float(params.loss_scale))
        return loss.sum()
