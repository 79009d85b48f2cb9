"""Trainer(..., envmap=...) on an MI355X: a 16 x 8 map, 256 rays, a tiny synthetic dataset of opaque images, max_samples 2^14.

What "bit for bit" is asserted on.  The envmap's path has no float atomic and the loss of a step is computed before that step's backward pass, so the loss, the
envmap's texels, its EMA and dL/doutput are functions of their inputs and are compared in every bit at the default learning rates.  The network's backward pass sums
parameter gradients with float atomics ("the last bits depend on the order of arrival", DESIGN.md "The backward pass"; tests/test_gpu_error_map.py and
tests/test_gpu_evaluate.py meet the same fact), so two identical steps need not leave the same last bit in every network weight, with or without an envmap.  The
network's parameters are therefore compared in every bit at network learning rate 0, where a step is a function of its inputs -- over TWO steps, so that the second
step's loss sees the first step's envmap update and anything the envmap's calls could have disturbed -- and at the default learning rate the number of differing
master weights after one step is printed, with no bar."""
import math

import numpy as np
import pytest
import torch

from training_rig import N_IMAGES, N_RAYS, RES, after_step, bits, by_hand, envmap_state, make_rig, make_trainer, step_rays

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def rig(built):
    return make_rig()


def test_step_is_the_calls_made_by_hand(rig):
    from nerfshop_amd import _abi
    # the default learning rates: loss, dL/doutput and the envmap in every bit; the network's weights counted
    a, b = make_trainer(rig, envmap=RES), make_trainer(rig, envmap=RES)
    rays, jitter, target, background, _ = step_rays(rig[2], a, want_pixels=False)
    loss_a = a.step(rays, target, jitter=jitter, background=background)
    loss_b, dl_b = by_hand(b, [0], rays, target, jitter, background)
    torch.cuda.synchronize()
    assert math.isfinite(float(loss_a)) and float(loss_a) > 0 and bits(loss_a) == bits(loss_b)
    assert bits(a._bufs.dl) == bits(dl_b), "dL/doutput: what the backward pass is given"
    assert envmap_state(a) == envmap_state(b)
    tex = a.envmap.get(_abi.ENVMAP_TEXELS)
    assert (tex[..., :3] != 0).sum() >= 12 and (tex[..., 3] == 0).all() and not a.envmap.get(_abi.ENVMAP_CELLS).any(), "the envmap moved, alpha did not, the cells are clear"
    assert a.envmap.step_count() == 1 and a.training_step == b.training_step == 1
    wa, wb = a.optimizer.get_state(_abi.OPT_MASTER), b.optimizer.get_state(_abi.OPT_MASTER)
    print(f"default learning rate: {int((wa.view(np.uint32) != wb.view(np.uint32)).sum())} of {wa.size} master weights differ in a bit after one step (float atomics of the backward pass)")
    # network learning rate 0: two steps, everything in every bit
    a, b = make_trainer(rig, envmap=RES, learning_rate=0.0), make_trainer(rig, envmap=RES, learning_rate=0.0)
    for k in range(2):
        rays, jitter, target, background, _ = step_rays(rig[2], a, want_pixels=False)
        loss_a = a.step(rays, target, jitter=jitter, background=background)
        loss_b, _ = by_hand(b, [0], rays, target, jitter, background)
        after_step((a, b))
        torch.cuda.synchronize()
        assert bits(loss_a) == bits(loss_b), k
    assert envmap_state(a) == envmap_state(b)
    for which in (_abi.OPT_MASTER, _abi.OPT_PARAMS_FP16):
        assert a.optimizer.get_state(which).tobytes() == b.optimizer.get_state(which).tobytes()


def test_an_envmap_that_is_never_reached_changes_nothing(rig):
    """Every ray stops -- raw densities of 12 under the exponential activation in a full occupancy grid: the first sample is opaque -- so no ray sees the background,
    accumulate deposits nothing, and a Trainer with an envmap computes what a Trainer without one computes: the losses and dL/doutput in every bit at the default
    learning rate, the network's parameters in every bit at learning rate 0 (module docstring)."""
    from nerfshop_amd import _abi, synth
    ctx, desc, ds, _ = rig
    weights = synth.make_params(desc, sigma_raw=12.0, density_noise=0.0).view(np.float16).astype(f32)
    full = np.ones(_abi.GRID_VOLUME * _abi.GRID_CASCADES, f32)
    from nerfshop_amd.trainer import Trainer
    for lr in (_abi.BASE_LEARNING_RATE, 0.0):
        plain = Trainer(ctx, desc, seed=11, weights=weights, density_grid=full, max_samples=1 << 14, learning_rate=lr)
        with_env = Trainer(ctx, desc, seed=11, weights=weights, density_grid=full, max_samples=1 << 14, learning_rate=lr, envmap=RES)
        for k in range(3 if lr == 0.0 else 1):
            la, lb = plain.step_dataset(ds, N_RAYS), with_env.step_dataset(ds, N_RAYS)
            torch.cuda.synchronize()
            assert math.isfinite(float(la)) and float(la) > 0 and bits(la) == bits(lb), (lr, k)
            live = int((with_env._bufs.aux[:, 10] > 0).sum())   # the emitted rays: every one has samples, and rows at or past the counter are never written
            assert bits(plain._bufs.dl) == bits(with_env._bufs.dl) and bits(plain._bufs.numsteps_out[:live]) == bits(with_env._bufs.numsteps_out[:live])
        aux = with_env._bufs.aux.cpu().numpy().view(np.uint32)
        assert (aux[:, 11] <= aux[:, 10]).all() and (aux[:, 10] > 0).sum() >= 8, "rays were emitted"
        n, M = aux[:, 10], aux[:, 11]
        T = aux[:, 3].copy().view(f32)
        assert ((M < n) | (n == 0) | (T == 0)).all(), "every ray stops, or (a ray of one sample) ends on a transmittance of exactly 0"
        assert not with_env.envmap.get(_abi.ENVMAP_CELLS).any() and not with_env.envmap.get(_abi.ENVMAP_TEXELS).any(), "nothing reached the envmap"
        assert with_env.envmap.step_count() == with_env.training_step
        if lr == 0.0:
            for which in (_abi.OPT_MASTER, _abi.OPT_PARAMS_FP16):
                assert plain.optimizer.get_state(which).tobytes() == with_env.optimizer.get_state(which).tobytes()


def test_the_envmap_learns_the_background(rig):
    """With the network's learning rate 0 only the envmap can lower the loss: over 32 steps on flat-coloured opaque images seen through a network that is still half
    transparent, the mean loss of the last 8 steps is below that of the first 8."""
    from nerfshop_amd import _abi
    t = make_trainer(rig, envmap=RES, learning_rate=0.0)
    before = t.optimizer.get_state(_abi.OPT_MASTER).tobytes()
    losses = torch.stack([t.step_dataset(rig[2], N_RAYS, random_bg=False) for _ in range(32)]).cpu().numpy()
    assert np.isfinite(losses).all() and (losses > 0).all()
    first, last = float(losses[:8].mean()), float(losses[-8:].mean())
    print(f"envmap alone: mean loss of steps 1-8 {first:.5f}, of steps 25-32 {last:.5f}")
    assert last < first
    assert t.optimizer.get_state(_abi.OPT_MASTER).tobytes() == before, "the network stood still"
    tex = t.envmap.get(_abi.ENVMAP_TEXELS)
    assert np.abs(tex[..., :3]).max() > 0.05 and (tex[..., 3] == 0).all() and t.envmap.step_count() == 32


def test_evaluate_renders_the_exported_texels(rig):
    from nerfshop_amd import runtime
    ctx, desc, ds, _ = rig
    t = make_trainer(rig, envmap=RES)
    for _ in range(4):
        t.step_dataset(ds, N_RAYS, random_bg=False)
    summary, records = t.evaluate(ds, spp=2)
    tb = runtime.Testbed(ctx, desc, network=t.network)
    tb.cone_angle_constant = t.cone_angle_constant
    tb.envmap = t.envmap.export(ema=False)
    _, by_hand_records = tb.evaluate(t.network, ds, spp=2)
    assert records.tobytes() == by_hand_records.tobytes()
    tb.envmap = None
    _, without = tb.evaluate(t.network, ds, spp=2)
    assert records.tobytes() != without.tobytes(), "the envmap is in the picture"
    # ema=True: the EMA texels behind the EMA network
    _, records_ema = t.evaluate(ds, ema=True, spp=2)
    assert torch.equal(t._eval_testbed.envmap, t.envmap.export(ema=True)) and not torch.equal(t.envmap.export(ema=True), t.envmap.export(ema=False))
    assert all(math.isfinite(v) for v in summary.values()) and len(records_ema) == N_IMAGES
