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

    def forward(self, coords):
        if coords.dim() != 2 or coords.shape[1] != 7:
            raise NrsError("NerfNetworkModule: input must be [n, 7]")
        return _NerfNetworkFunction.apply(self.params, coords.contiguous(), self)
