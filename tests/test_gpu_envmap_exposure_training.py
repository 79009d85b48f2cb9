"""Trainer(..., envmap=..., exposure=...) on an MI355X: both side parameters in one step, on training_rig's rig -- 4 images of 16 x 12, 256 rays, max_samples 2^14, a
16 x 8 map.  This is the configuration in which the per-slot record of the loss (aux) is written once and read by both gradients, and in which the envmap's and
the exposure's calls interleave around the loss and behind the optimiser.

What "bit for bit" is asserted on is what tests/test_gpu_envmap_training.py and tests/test_gpu_exposure_training.py assert it on, for both parameters at once: neither
path has a float atomic and a step's loss is computed before its backward pass, so the loss, dL/doutput, the envmap's state and the exposure's state are functions
of their inputs.  At the default learning rates ONE step with cam_update_every = 1 (the exposure's update falls inside it) is compared in all of them; at network
learning rate 0, where the float atomics of the backward pass cannot reach the weights, 17 steps with the default cadence (the update falls on the 16th) are compared
in all of them step by step, and the network's master and fp16 parameters behind them."""
import math

import numpy as np
import pytest
import torch

import training_rig
from training_rig import N_IMAGES, RES, after_step, bits, by_hand, envmap_state, exposure_state, make_trainer, new_exposure

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def rig(built):
    return training_rig.make_rig()


def test_step_with_both_is_the_calls_made_by_hand(rig):
    from nerfshop_amd import _abi
    ds = rig[2]
    start = np.random.default_rng(2).uniform(-1.0, 1.0, (N_IMAGES, 3)).astype(f32)
    # the default learning rates, an update on every step: one step, the envmap and the exposures move
    a, b = (make_trainer(rig, envmap=RES, exposure=new_exposure(rig, start), cam_update_every=1) for _ in range(2))
    rays, jitter, target, background, pixels = training_rig.step_rays(ds, a, want_pixels=True)
    loss_a = a.step(rays, target, jitter=jitter, background=background, pixels=pixels)
    loss_b, dl_b = by_hand(b, [0], rays, target, jitter, background, pixels)
    torch.cuda.synchronize()
    assert math.isfinite(float(loss_a)) and float(loss_a) > 0 and bits(loss_a) == bits(loss_b)
    assert bits(a._bufs.dl) == bits(dl_b), "dL/doutput: what the backward pass is given"
    assert envmap_state(a) == envmap_state(b) and exposure_state(a) == exposure_state(b)
    tex = a.envmap.get(_abi.ENVMAP_TEXELS)
    assert (tex[..., :3] != 0).sum() >= 12 and not a.envmap.get(_abi.ENVMAP_CELLS).any() and a.envmap.step_count() == 1, "the envmap moved, its cells are clear"
    assert (a.exposures() != start).all() and not a.exposure.get(_abi.EXPOSURE_CELLS).any() and a.exposure.step_count() == 1, "the exposures moved, their cells are clear"
    # network learning rate 0, the default cadence: 17 steps, everything in every bit
    a, b = (make_trainer(rig, learning_rate=0.0, envmap=RES, exposure=new_exposure(rig, start)) for _ in range(2))
    hand = [0]
    for k in range(17):
        rays, jitter, target, background, pixels = training_rig.step_rays(ds, a, want_pixels=True)
        loss_a = a.step(rays, target, jitter=jitter, background=background, pixels=pixels)
        loss_b, dl_b = by_hand(b, hand, rays, target, jitter, background, pixels)
        after_step((a, b))
        torch.cuda.synchronize()
        assert bits(loss_a) == bits(loss_b) and bits(a._bufs.dl) == bits(dl_b), k
        assert envmap_state(a) == envmap_state(b) and exposure_state(a) == exposure_state(b), k
        assert a.envmap.step_count() == k + 1 and a.exposure.step_count() == (1 if k >= 15 else 0), "the envmap steps every time, the exposures on the 16th step"
    assert a.envmap.get(_abi.ENVMAP_TEXELS).any() and a.exposure.get(_abi.EXPOSURE_M).any(), "both updates ran"
    for which in (_abi.OPT_MASTER, _abi.OPT_PARAMS_FP16):
        assert a.optimizer.get_state(which).tobytes() == b.optimizer.get_state(which).tobytes()
