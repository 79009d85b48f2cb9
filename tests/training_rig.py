"""What the Trainer's side-parameter tests share (test_gpu_envmap_training.py, test_gpu_exposure_training.py, test_gpu_envmap_exposure_training.py): a tiny synthetic
dataset of opaque images -- 4 images of 16 x 12, 256 rays a step, max_samples 2^14, a 16 x 8 environment map -- the rays a dataset step would draw, and the training
step stated by hand.

by_hand is the yardstick Trainer.step is compared with, so it stays independent of the trainer's own step: it calls runtime objects only (the trainer's network,
optimiser, envmap and exposure, which ARE the state under test) and allocates every tensor itself -- never the trainer's buffers, never its side-parameter code."""
import math

import numpy as np
import torch

W, H, N_IMAGES, N_RAYS, RES = 16, 12, 4, 256, (16, 8)
COLOURS = [(230, 160, 60), (60, 200, 120), (90, 110, 240), (200, 200, 200)]


def make_dataset(ctx, colours):
    from nerfshop_amd import _abi, runtime, synth
    focal = 0.5 * W / math.tan(0.5 * synth.CAMERA_ANGLE_X)
    ds = runtime.Dataset(ctx, len(colours), W, H)
    for k, colour in enumerate(colours):
        img = np.empty((H, W, 4), np.uint8)
        img[..., :3], img[..., 3] = colour, 255    # opaque: the target is the image's colour whatever lies behind it
        ds.set_image(k, img)
        cam = _abi.TrainingCamera()
        cam.xform_start[:] = cam.xform_end[:] = synth.orbit_camera(40.0 + 90.0 * k).tolist()
        cam.focal_length[:], cam.principal_point[:] = (focal, focal), (0.5, 0.5)
        ds.set_camera(k, cam)
    return ds


def make_rig():
    """(ctx, desc, dataset, density grid): what a module's `rig` fixture returns"""
    from nerfshop_amd import runtime, synth
    ctx = runtime.Context(0)
    return ctx, synth.model_desc(log2_hashmap_size=14), make_dataset(ctx, COLOURS), synth.density_grid(1)


def make_trainer(rig, **kw):
    from nerfshop_amd.trainer import Trainer
    ctx, desc, _, grid = rig
    return Trainer(ctx, desc, seed=11, density_grid=grid, max_samples=1 << 14, **kw)


def new_exposure(rig, values=None, n_images=N_IMAGES, **params):
    from nerfshop_amd import _abi, runtime
    exp = runtime.Exposure(rig[0], n_images, _abi.ExposureParams(**params))
    if values is not None:
        exp.set(values)
    return exp


def step_rays(ds, trainer, want_pixels):
    """the rays Trainer.step_dataset would draw at the trainer's state: (rays, jitter, target, background, pixels -- None unless wanted)"""
    u = trainer._grid_update
    return ds.rays(N_RAYS, trainer.n_rays_total, (u.rng_state, u.rng_inc), snap=True, random_bg=True, want_pixels=want_pixels)


def after_step(trainers):
    """what step_dataset does behind a step"""
    from nerfshop_amd import runtime
    for t in trainers:
        t.n_rays_total += N_RAYS
        t._grid_update.rng_state = runtime.rng_advance(t._grid_update.rng_state, t._grid_update.rng_inc)


def by_hand(t, hand, rays, target, jitter, background, pixels=None):
    """The calls of one training step, in Trainer._step's order, for whatever side parameters the trainer `t` has: none, an envmap, an exposure or both.  hand: the
    steps accumulated since the exposure's last update (a one-element list).  Returns (loss, dL/doutput as handed to the backward pass)."""
    from nerfshop_amd import _abi
    net, env, expo, p = t.network, t.envmap, t.exposure, t.loss_params
    n = int(rays.shape[0])
    coords, numsteps, ray_indices, counters = net.training_samples(None, rays, jitter, t.cone_angle_constant, t.max_samples)
    net.inference_strided(None, coords, t._out16)
    counter, slots = counters[:1], ray_indices.to(torch.int64)
    if expo is None:
        target_s = target.index_select(0, slots)
    else:
        target_s, scale = expo.targets(ray_indices, counter, pixels, target)
    bg_s = background.index_select(0, slots)
    bg_linear = footprint = None
    if env is not None:
        bg_linear, footprint = env.background(rays, ray_indices, counter, background=bg_s, default_background=tuple(p.background))
    aux = None if env is None and expo is None else torch.zeros((n, _abi.RAY_AUX_WORDS), dtype=torch.int32, device=rays.device)
    numsteps_out, coords_out, dl, loss, _ = net.ray_loss(None, p, numsteps, coords, t._out16, target_s, background=bg_s, ray_counter=counter,
                                                         background_linear=bg_linear, aux=aux)
    if env is not None:
        acc = _abi.EnvmapAccumulateParams(p.loss_type, t.envmap_loss_type, p.loss_scale, p.train_in_linear_colors)
        env.accumulate(acc, counter, numsteps_out, aux, bg_linear, footprint, n_rays=n)
    if expo is not None:
        expo.accumulate(_abi.ExposureAccumulateParams(p.loss_scale, p.train_in_linear_colors), counter, ray_indices, numsteps_out, aux, scale, n_rays=n)
    net.backward(None, coords_out, dl, t.grad, None, accumulate=True)
    t.optimizer.step(t.grad, loss_scale=float(p.loss_scale), lr=t.current_learning_rate(), zero_grad=True)
    if env is not None:
        env.step(loss_scale=float(p.loss_scale), lr=t.current_envmap_learning_rate())
    if expo is not None:
        hand[0] += 1
        if hand[0] >= t.cam_update_every:
            expo.step(loss_scale=float(p.loss_scale), lr=t.current_learning_rate())
            hand[0] = 0
    t.training_step += 1
    return loss.sum(), dl


def bits(x):
    return x.detach().cpu().numpy().tobytes() if isinstance(x, torch.Tensor) else np.ascontiguousarray(x).tobytes()


def envmap_state(t):
    from nerfshop_amd import _abi
    return [t.envmap.get(w).tobytes() for w in (_abi.ENVMAP_TEXELS, _abi.ENVMAP_EMA, _abi.ENVMAP_CELLS)]


def exposure_state(t):
    from nerfshop_amd import _abi
    return [t.exposure.get(w).tobytes() for w in (_abi.EXPOSURE_VALUES, _abi.EXPOSURE_M, _abi.EXPOSURE_V, _abi.EXPOSURE_CELLS)] + [t.exposure.step_count()]
