"""nrs_optimizer (nrs_api_optimizer.cpp): the fused Adam step and the host functions of its schedule."""
import ctypes as C

import numpy as np
import torch

from .. import _abi
from .._abi import NrsError, check
from ._base import Handle, _device, _require_cuda, _stream_handle


class Optimizer(Handle):
    """tiny-cuda-nn's Adam (per-parameter step counts, zero-gradient skip, L2 on the matrix weights) with the EMA of base.json, one fused HIP kernel per step
    (nrs_optimizer_*).  Optimizer(ctx, n_params=..., n_matrix=...) keeps an fp16 array of its own; Optimizer(ctx, network=net) is bound to a NerfNetwork: a step
    writes the network's resident hash table in place and refreshes its MLP fragments on the same stream, so the next forward pass reads the new parameters with no
    copy.  The network must outlive the optimiser."""

    _destroy = "nrs_optimizer_destroy"
    _DTYPES = {_abi.OPT_MASTER: np.float32, _abi.OPT_M: np.float32, _abi.OPT_V: np.float32, _abi.OPT_STEPS: np.uint32, _abi.OPT_EMA: np.float32,
               _abi.OPT_PARAMS_FP16: np.float16}

    def __init__(self, ctx, n_params=None, n_matrix=0, network=None, params=None):
        super().__init__(ctx.lib)
        self.ctx, self.network = ctx, network
        self.params = params if params is not None else _abi.AdamParams()
        if not isinstance(self.params, _abi.AdamParams):
            raise NrsError("Optimizer: params must be an AdamParams")
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
            out = torch.empty(self.n_params, dtype=torch.float16, device=_device(self.ctx))
        _require_cuda(out, torch.float16, "out")
        if out.numel() != self.n_params:
            raise NrsError(f"Optimizer.export_fp16: out must hold {self.n_params} elements")
        check(self.lib.nrs_optimizer_export_fp16(self.h, int(which), out.data_ptr(), _stream_handle(stream)))
        return out


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
