"""The backward pass without a GPU: the reference twin itself is checked (its forward against the oracle, its autograd against central differences), and the
library's new surface exists and validates its arguments before it touches a device."""
import ctypes as C

import numpy as np
import pytest
import torch

import network_backward_ref as ref


@pytest.fixture(scope="module")
def setup(built):
    from nerfshop_amd import synth
    desc = synth.model_desc(1, log2_hashmap_size=14)
    lt = ref.level_table(desc)
    p16 = ref.make_params(desc, 7)
    coords = ref.make_coords(np.random.default_rng(3), 777)
    return desc, lt, p16, coords


def test_twin_forward_against_oracle(setup):
    from oracle import oracle as orc
    desc, lt, p16, coords = setup
    assert p16.size == 501520
    want = orc.Model(desc, p16.view(np.uint16)).inference(coords, layout=1).view(np.float16).astype(np.float64)
    got = ref.forward(lt, torch.from_numpy(p16.astype(np.float64)), coords).numpy()
    diff = np.abs(got - want)
    ulp = np.spacing(np.abs(want).astype(np.float16)).astype(np.float64)  # the fp16 step at the oracle's value
    frac, worst = float((diff > 0).mean()), float((diff / ulp).max())
    print(f"twin vs oracle: {int((diff > 0).sum())} of {diff.size} outputs differ, by at most {worst:.2f} fp16 ulps")
    assert frac <= 0.005
    assert worst <= 4.0


def test_twin_autograd_against_central_differences(setup):
    desc, lt, p16, coords = setup
    rng = np.random.default_rng(5)
    DL = torch.zeros(777, 16, dtype=torch.float64)
    DL[:, :4] = torch.from_numpy(rng.normal(size=(777, 4)))

    def loss(P):
        return (ref.forward(lt, P, coords, rounding=ref.identity) * DL).sum()

    P0 = torch.from_numpy(p16.astype(np.float64)).requires_grad_(True)
    g, = torch.autograd.grad(loss(P0), P0)
    v = torch.from_numpy(rng.normal(size=P0.numel()))
    eps = 1e-6
    fd = ((loss(P0.detach() + eps * v) - loss(P0.detach() - eps * v)) / (2 * eps)).item()
    ad = (g * v).sum().item()
    print(f"directional derivative: autograd {ad:.9e} central difference {fd:.9e}")
    assert abs(ad - fd) <= 1e-8 * abs(fd)


def test_surface_exists(built):
    from nerfshop_amd import _abi, runtime
    lib = _abi.load()
    assert hasattr(lib, "nrs_network_backward")
    assert "nrs_network_backward" in _abi.EXPORTS
    assert callable(getattr(runtime.NerfNetwork, "backward", None))
    from nerfshop_amd import torch_module
    assert issubclass(torch_module.NerfNetworkModule, torch.nn.Module)
    # the initialisation is a function of the seed: Xavier-uniform matrices, U(-1e-4, 1e-4) grid
    a, b = torch_module.initial_params(20000, 11), torch_module.initial_params(20000, 11)
    assert torch.equal(a, b) and not torch.equal(a, torch_module.initial_params(20000, 7))
    assert a.dtype == torch.float32 and float(a[ref.N_MLP:].abs().max()) <= 1e-4
    assert float(a[:2048].abs().max()) <= (6.0 / 96.0) ** 0.5 and float(a[:2048].abs().max()) > 0.2


def test_null_arguments_are_refused_without_a_device(built):
    from nerfshop_amd import _abi
    lib = _abi.load()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    INVALID = -1
    # no model; then (a fake non-NULL model is never dereferenced before the NULL checks) each buffer in turn
    assert lib.nrs_network_backward(None, None, 1, p, 7, p, 1, 0, p, 1, 0, None) == INVALID
    assert b"NULL" in lib.nrs_last_error()
    fake = C.c_void_p(p)
    assert lib.nrs_network_backward(fake, None, 1, None, 7, p, 1, 0, p, 1, 0, None) == INVALID
    assert lib.nrs_network_backward(fake, None, 1, p, 7, None, 1, 0, p, 1, 0, None) == INVALID
    assert lib.nrs_network_backward(fake, None, 1, p, 7, p, 1, 0, None, 1, 0, None) == INVALID
