"""The reference's training loop from the ray on, end to end on the device: samples -> inference -> ray loss -> backward -> the fused optimiser step,
with an optional trained environment map behind the last sample (Trainer(..., envmap=(256, 128))) and an optional trained exposure per training image
(Trainer(..., exposure=True)).

    trainer = Trainer(ctx, synth.model_desc(1), seed=11, density_grid=grid)      # or no grid: the first update_density_grid() makes one from the network
    for i in range(n_steps):
        if i % 16 == 0:
            trainer.update_density_grid()
        loss = trainer.step(rays, target_rgba)          # rays [n, 6] f32 (origin, unit direction), target_rgba [n, 4] f32 linear premultiplied; CUDA tensors
    ema_blob = trainer.optimizer.export_fp16(_abi.OPT_EXPORT_EMA)                 # what a second NerfNetwork renders with (set_params_device)

or, from posed images (a transforms.json folder):

    ds = dataset.load_transforms("data/nerf/fox").to_device(ctx)                  # runtime.Dataset
    losses = trainer.fit(ds, n_steps=1000)                                        # mark_untrained + grid updates every 16 steps + step_dataset

Everything in `step` is enqueued on the current stream and nothing is read back: the loss comes back as a 0-d tensor on the device.  The optimiser is
configs/nerf/base.json's -- Ema(0.95) over ExponentialDecay(20000, 10000, 0.33) over Adam(1e-2, 0.9, 0.99, 1e-15, l2_reg 1e-6) -- and writes the network's parameters
in place (runtime.Optimizer bound to the network), so no set_params call and no gradient memset sits between two steps.
"""
import numpy as np
import torch

from . import _abi, runtime
from ._abi import NrsError
from .torch_module import LOSS_SCALE, initial_params


class ErrorMapSchedule:
    """train_nerf's error map for Trainer.step_dataset / fit, with the reference's cadence (src/testbed_nerf.cu:3724-3830): every step's ray losses are deposited
    into the dataset's error map; after steps_between steps (128, the reference's n_steps_between_error_map_updates) the map becomes CDFs and steps_between
    becomes (uint32)(steps_between * growth) (1.5); the step after a build starts a fresh map.  sample_images / sample_pixels
    (sample_image_proportional_to_error / sample_focal_plane_proportional_to_error, both off in the reference's Testbed) draw the next steps' images / pixels
    from those CDFs once a build has happened.  The object carries the state: steps_between (current), steps_since (the last build), builds, build_steps (the
    trainer's training_step after each build), resolution (of the current map); keep_last=True also keeps clones of each step's (ray_counter, ray_indices, loss) as
    last_loss beside last_rays = (xy, pixels, pdf), for inspection."""

    def __init__(self, steps_between=128, growth=1.5, sample_images=False, sample_pixels=False, keep_last=False):
        if int(steps_between) < 1 or not float(growth) >= 1.0:
            raise NrsError("ErrorMapSchedule: steps_between must be at least 1 and growth at least 1")
        self.steps_between, self.growth = int(steps_between), float(growth)
        self.sample_images, self.sample_pixels, self.keep_last = bool(sample_images), bool(sample_pixels), bool(keep_last)
        self.steps_since, self.builds, self.build_steps = 0, 0, []
        self.resolution, self.last_rays, self.last_loss = None, None, None


class _RayBuffers:
    """Every tensor of a step whose size follows n_rays, made here and re-made only when n_rays changes: the five of NerfNetwork.ray_loss_buffers; aux [n, RAY_AUX_WORDS],
    the per-slot record of the loss that both side gradients read, when there is a side parameter; the envmap's background_linear and footprint; the exposure's target
    and scale.  What a side parameter reads by slot is made zero: rows at or past the ray counter are never written."""

    def __init__(self, net, n_rays, max_samples, device, envmap, exposure):
        def zeros(width, dtype):
            return torch.zeros((n_rays, width), dtype=dtype, device=device)
        self.n_rays = n_rays
        self.numsteps_out, self.coords_out, self.dl, self.loss, self.counter = net.ray_loss_buffers(n_rays, max_samples, device=device)
        self.aux = zeros(_abi.RAY_AUX_WORDS, torch.int32) if envmap or exposure else None
        self.background_linear, self.footprint = (zeros(3, torch.float32), zeros(4, torch.int32)) if envmap else (None, None)
        self.target, self.scale = (zeros(4, torch.float32), zeros(4, torch.int32)) if exposure else (None, None)


class _Envmap:
    """What the trainer `t` knows about its environment map (m_envmap), whose state is t's own -- t.envmap, t.envmap_loss_type (base.json's envmap loss),
    t.envmap_learning_rate and t.envmap_decay (its schedule): in front of the loss the background a ray sees through the live texels, and the lookup's footprint for
    the gradient; behind the loss the gradient's deposits; behind the network's step the texels'."""

    def __init__(self, t, envmap, loss_type, learning_rate, decay):
        if envmap is not None and not isinstance(envmap, runtime.Envmap):
            envmap = runtime.Envmap(t.ctx, int(envmap[0]), int(envmap[1]))
        if envmap is not None and envmap.ctx is not t.ctx:
            raise NrsError("Trainer: the envmap belongs to another context")
        self.t, t.envmap, t.envmap_loss_type, t.envmap_learning_rate, t.envmap_decay = t, envmap, int(loss_type), float(learning_rate), tuple(decay)

    def before_loss(self, b, rays, ray_indices, counter, background):
        self.t.envmap.background(rays, ray_indices, counter, background=background, default_background=tuple(self.t.loss_params.background),
                                 out=(b.background_linear, b.footprint))

    def after_loss(self, b, ray_indices, counter, xy_pdf):
        t, p = self.t, self.t.loss_params
        acc = _abi.EnvmapAccumulateParams(p.loss_type, t.envmap_loss_type, p.loss_scale, p.train_in_linear_colors)
        t.envmap.accumulate(acc, counter, b.numsteps_out, b.aux, b.background_linear, b.footprint, n_rays=b.n_rays)

    def after_optimizer(self):
        self.t.envmap.step(loss_scale=float(self.t.loss_params.loss_scale), lr=self.t.current_envmap_learning_rate())


class _Exposure:
    """What the trainer `t` knows about its per-image exposures (m_nerf.training.optimize_exposure), whose state is t's own -- t.exposure (None, a runtime.Exposure, or
    True until the first dataset step, which knows the number of images, makes one), t.exposure_l2_reg, t.cam_update_every: what a dataset step and a step refuse; in
    front of the loss the targets by slot (the gather and the image's 2^exposure in one pass; the scale is kept for the gradient); behind the loss the gradient's
    deposits; and the camera update of train_nerf (src/testbed_nerf.cu:3834-3915) on the step on which cam_update_every of them have been accumulated, with the
    network's learning rate."""

    def __init__(self, t, exposure, l2_reg, update_every):
        if exposure is not None and exposure is not True and not isinstance(exposure, runtime.Exposure):
            raise NrsError("Trainer: exposure must be None, True or a runtime.Exposure")
        if isinstance(exposure, runtime.Exposure) and exposure.ctx is not t.ctx:
            raise NrsError("Trainer: the exposure belongs to another context")
        if int(update_every) < 1:
            raise NrsError("Trainer: cam_update_every must be at least 1")
        self.t, t.exposure, t.exposure_l2_reg, t.cam_update_every, self.steps_since_update = t, exposure, float(l2_reg), int(update_every), 0

    def before_dataset_step(self, dataset, error_map):
        t = self.t
        if error_map is not None and error_map.sample_images and error_map.sample_pixels:
            raise NrsError("Trainer.step_dataset: exposure with sample_images and sample_pixels: the exposure's gradient is divided by the pixel's density alone, "
                           "but the dataset writes the product of the image's and the pixel's, and the two cannot be told apart")
        if t.exposure is True:
            t.exposure = runtime.Exposure(t.ctx, dataset.n_images, _abi.ExposureParams(l2_reg=t.exposure_l2_reg, steps_between_updates=t.cam_update_every))
        elif t.exposure.n_images != dataset.n_images:
            raise NrsError("Trainer.step_dataset: the exposure was made for another number of images")

    def before_step(self, pixels):
        if pixels is None:
            raise NrsError("Trainer.step: with an exposure, `pixels` must name each ray's image")
        if self.t.exposure is True:
            raise NrsError("Trainer.step: exposure=True is made by the first step_dataset, which knows the number of images; pass a runtime.Exposure to step() directly")

    def before_loss(self, b, ray_indices, counter, pixels, target_rgba):
        self.t.exposure.targets(ray_indices, counter, pixels, target_rgba, out=(b.target, b.scale))

    def after_loss(self, b, ray_indices, counter, xy_pdf):
        p = self.t.loss_params
        self.t.exposure.accumulate(_abi.ExposureAccumulateParams(p.loss_scale, p.train_in_linear_colors), counter, ray_indices, b.numsteps_out, b.aux, b.scale,
                                   xy_pdf=xy_pdf, n_rays=b.n_rays)

    def after_optimizer(self):
        self.steps_since_update += 1
        if self.steps_since_update >= self.t.cam_update_every:
            self.t.exposure.step(loss_scale=float(self.t.loss_params.loss_scale), lr=self.t.current_learning_rate())
            self.steps_since_update = 0


class Trainer:
    """A NerfNetwork without cell records, an Optimizer bound to it, one persistent gradient buffer (zero between steps: the optimiser clears what it reads) and
    base.json's learning-rate schedule.

        trainer = Trainer(ctx, desc, seed=11, density_grid=synth.density_grid(1))
        losses = [trainer.step(rays, target_rgba) for _ in range(16)]          # 0-d CUDA tensors; float(losses[-1]) waits for the device
        trainer.update_density_grid()
    """

    def __init__(self, ctx, desc, seed=1337, weights=None, density_grid=None, max_samples=1 << 18, max_cascade=0, cone_angle_constant=0.0, adam=None,
                 loss_params=None, learning_rate=_abi.BASE_LEARNING_RATE, decay=(_abi.BASE_DECAY_START, _abi.BASE_DECAY_INTERVAL, _abi.BASE_DECAY_BASE),
                 density_grid_decay=0.95, envmap=None, envmap_loss_type=_abi.LOSS_RELATIVE_L2, envmap_learning_rate=_abi.ENVMAP_LEARNING_RATE,
                 envmap_decay=(_abi.ENVMAP_DECAY_START, _abi.ENVMAP_DECAY_INTERVAL, _abi.ENVMAP_DECAY_BASE), exposure=None, exposure_l2_reg=0.0, cam_update_every=16):
        """envmap: None, a runtime.Envmap or a (res_x, res_y) pair: an environment map trained next to the network (m_envmap) -- the background behind a ray's last
        sample, with base.json's envmap loss (RelativeL2) and its own schedule, ExponentialDecay(10000, 5000, 0.33) over 1e-2, on training_step.
        exposure: None, True or a runtime.Exposure: a log2 exposure per training image and channel, trained next to the network (m_nerf.training.optimize_exposure).
        True makes one on the first step_dataset, when the number of images is known, with exposure_l2_reg and cam_update_every (the reference's exposure_l2_reg and
        n_steps_between_cam_updates) as its l2_reg and steps_between_updates; a runtime.Exposure brings its own parameters.  Every step deposits the exposure's
        gradient; the step on which cam_update_every of them have been accumulated runs Exposure.step with the network's current learning rate.  exposures() returns
        the values: a training view is displayed with the tonemap's exposure + exposures()[view]."""
        self.ctx, self.lib, self.desc = ctx, ctx.lib, desc
        self._expo = _Exposure(self, exposure, exposure_l2_reg, cam_update_every)  # (each sets its part of the trainer's state)
        self._env = _Envmap(self, envmap, envmap_loss_type, envmap_learning_rate, envmap_decay)
        self._bufs = None  # _RayBuffers: made by the first step
        self.network = runtime.NerfNetwork(ctx, desc, cell_cache_bytes=0)  # no cell-record cache: it would be rebuilt after every step
        self.optimizer = runtime.Optimizer(ctx, network=self.network, params=adam)
        n = self.optimizer.n_params
        dev = f"cuda:{ctx.device}"
        self.optimizer.set_weights(weights if weights is not None else initial_params(n, seed).numpy())
        self.grad = torch.zeros(n, dtype=torch.float32, device=dev)
        self.max_samples, self.cone_angle_constant = int(max_samples), float(cone_angle_constant)
        self.loss_params = loss_params if loss_params is not None else _abi.RayLossParams(loss_scale=LOSS_SCALE)
        self.loss_params.max_samples_compacted = self.max_samples
        self.learning_rate, self.decay = float(learning_rate), tuple(decay)
        self.training_step = 0
        self.n_rays_total = 0  # m_nerf.training.n_rays_total: rays drawn from a dataset so far (step_dataset)
        self._out16 = torch.empty((self.max_samples, 16), dtype=torch.float16, device=dev)
        self._grid_update = _abi.GridUpdate()
        self._grid_update.max_cascade, self._grid_update.ema_step = int(max_cascade), 0
        self._grid_update.rng_state, self._grid_update.rng_inc = runtime.rng_seed(seed)
        self.density_grid_decay = float(density_grid_decay)
        self._grid_step = 0  # the training step of the last update_density_grid
        self._eval_testbed, self._ema_network = None, None  # evaluate(): made on first use
        if density_grid is not None:
            self.network.set_density_grid(np.ascontiguousarray(density_grid, dtype=np.float32))
        else:
            self.update_density_grid()

    def current_learning_rate(self):
        start, interval, base = self.decay
        return runtime.exponential_decay_lr(self.training_step, self.learning_rate, start, interval, base)

    def current_envmap_learning_rate(self):
        start, interval, base = self.envmap_decay
        return runtime.exponential_decay_lr(self.training_step, self.envmap_learning_rate, start, interval, base)

    def update_density_grid(self, stream=None):
        """training_prep_nerf (src/testbed_nerf.cu:4460-4468): uniform samples over every cell while the training step is below 256, a quarter uniform plus a quarter
        non-uniform afterwards; the grid decays by 0.95^(k / 16) with k the steps since the last call (16 at the very first one, the reference's cadence)."""
        k = self.training_step - self._grid_step if self.training_step else 16
        u = self._grid_update
        cells = _abi.GRID_VOLUME * (u.max_cascade + 1)
        if self.training_step < 256:
            u.n_uniform_samples, u.n_nonuniform_samples = cells, 0
        else:
            u.n_uniform_samples, u.n_nonuniform_samples = cells // 4, cells // 4
        u.reset_grid = 0
        u.decay = self.density_grid_decay ** (k / 16.0)
        self.network.update_density_grid(u, stream=stream)
        self._grid_step = self.training_step

    def step(self, rays, target_rgba, jitter=None, background=None, pixels=None, xy_pdf=None):
        """One training step on rays [n, 6] f32 with the colours they should have, target_rgba [n, 4] f32 (linear, premultiplied); jitter [n] in [0, 1) or None,
        background [n, 3] (sRGB-encoded) or None for loss_params.background.  Returns the mean loss as a 0-d CUDA tensor.  Nothing waits for the device.
        With an exposure: pixels [n, 2] int32 (image, pixel) by ray names each ray's image (required), and xy_pdf [n] f32 by ray, or None for 1, is the density the
        pixel was drawn with inside its image -- the divisor of the exposure's gradient."""
        return self._step(rays, target_rgba, jitter, background, None, pixels, xy_pdf)

    def exposures(self):
        """The trained exposures [n_images, 3] f32 on the host (log2: a channel is scaled by 2^value), or None without an exposure or before the first dataset step
        has made one.  A training view is displayed with the tonemap's exposure + exposures()[view] (runtime.Testbed's tonemap parameter)."""
        return self.exposure.get() if isinstance(self.exposure, runtime.Exposure) else None

    def _step(self, rays, target_rgba, jitter, background, after_loss, pixels=None, xy_pdf=None):
        """step(); after_loss(ray_counter, ray_indices, loss), if given, runs between the ray loss and the backward pass and may rewrite the per-slot losses in place."""
        net, n_rays = self.network, int(rays.shape[0])
        if tuple(target_rgba.shape) != (n_rays, 4):
            raise NrsError("Trainer.step: target_rgba must be [n_rays, 4]")
        env, expo = self._env if self.envmap is not None else None, self._expo if self.exposure is not None else None
        sides = [side for side in (env, expo) if side]  # in the order of their calls behind the loss
        if expo:
            expo.before_step(pixels)
        coords, numsteps, ray_indices, counters = net.training_samples(None, rays, jitter, self.cone_angle_constant, self.max_samples)
        net.inference_strided(None, coords, self._out16)
        if self._bufs is None or self._bufs.n_rays != n_rays:
            self._bufs = _RayBuffers(net, n_rays, self.max_samples, rays.device, bool(env), bool(expo))
        b, counter = self._bufs, counters[:1]
        # the loss reads its per-ray inputs by ray SLOT: gather them with the generator's indices (slots at or past counters[0] are not live)
        slots = ray_indices.to(torch.int64)
        if expo:
            expo.before_loss(b, ray_indices, counter, pixels, target_rgba)
        target = b.target if expo else target_rgba.index_select(0, slots)
        bg = None if background is None else background.index_select(0, slots)
        if env:
            env.before_loss(b, rays, ray_indices, counter, bg)
        net.ray_loss(None, self.loss_params, numsteps, coords, self._out16, target, background=bg, ray_counter=counter,
                     out=(b.numsteps_out, b.coords_out, b.dl, b.loss, b.counter), background_linear=b.background_linear, aux=b.aux)
        if after_loss is not None:
            after_loss(counter, ray_indices, b.loss)
        for side in sides:
            side.after_loss(b, ray_indices, counter, xy_pdf)
        net.backward(None, b.coords_out, b.dl, self.grad, None, accumulate=True)
        self.optimizer.step(self.grad, loss_scale=float(self.loss_params.loss_scale), lr=self.current_learning_rate(), zero_grad=True)
        for side in sides:
            side.after_optimizer()
        self.training_step += 1
        return b.loss.sum()

    def step_dataset(self, dataset, n_rays=4096, snap=True, random_bg=True, error_map=None):
        """One training step on n_rays pixels of a runtime.Dataset: dataset.rays (image and pixel selection, the pixel's camera, lens distortion; the target colour and
        the random background the loss composites behind it) -> step().  The generator is the trainer's m_rng (the one update_density_grid draws from), advanced once per
        step by NRS_RNG_STEP_DELTA as the reference advances it (src/testbed_nerf.cu:4435); n_rays_total counts the rays of the steps before.  snap and random_bg
        default to the reference's Testbed initialisers (include/neural-graphics-primitives/testbed.h:584 and :581).  Like step, nothing waits for the device.
        error_map: an ErrorMapSchedule runs train_nerf's error map around the step (src/testbed_nerf.cu:3724-3831): the map is reset, at the resolution recomputed
        from the schedule, when no step has passed since the last build; the rays are drawn from the CDFs once there are valid ones and the schedule asks for it; every
        ray's loss is deposited after the ray loss (the returned loss is then the sum of loss / pdf, the loss the reference reports); and once steps_between steps have
        passed the CDFs are rebuilt and steps_between grows.  All on the device; with both sampling switches off the step computes what it computes without a schedule."""
        u, expo = self._grid_update, self.exposure is not None
        if expo:
            self._expo.before_dataset_step(dataset, error_map)
        draw = dict(n_rays=n_rays, n_rays_total=self.n_rays_total, rng=(u.rng_state, u.rng_inc), snap=snap, random_bg=random_bg)
        if error_map is None:
            rays, jitter, target, background, pixels = dataset.rays(**draw, want_pixels=expo)
            loss = self.step(rays, target, jitter=jitter, background=background, pixels=pixels)
        else:
            em = error_map
            if em.steps_since == 0:
                em.resolution = dataset.error_map_resolution(em.steps_between, n_rays)
                dataset.error_map_reset(*em.resolution)
            by_error = (em.sample_images and em.builds > 0, em.sample_pixels and em.builds > 0)  # (the reference hands the CDFs over only once is_cdf_valid)
            rays, jitter, target, background, pixels, xy, pdf = dataset.rays(**draw, by_error=by_error)
            em.last_rays = (xy, pixels, pdf)

            def accumulate(ray_counter, ray_indices, loss):
                em.last_loss = (ray_counter.clone(), ray_indices.clone(), loss.clone()) if em.keep_last else None
                dataset.error_map_accumulate(n_rays, ray_counter, ray_indices, loss, xy, pixels, pdf=pdf, loss_weighted=loss)
            # the exposure's divisor is xy_pdf alone (src/testbed_nerf.cu:1948): with images drawn uniformly the dataset's pdf is exactly that
            loss = self._step(rays, target, jitter, background, accumulate, pixels if expo else None, pdf if expo and by_error[1] else None)
            em.steps_since += 1
            if em.steps_since >= em.steps_between:
                dataset.error_map_build_cdfs()
                em.builds += 1
                em.build_steps.append(self.training_step)
                em.steps_since = 0
                em.steps_between = int(np.float32(em.steps_between) * np.float32(em.growth)) & 0xffffffff
        self.n_rays_total = (self.n_rays_total + int(n_rays)) & 0xffffffff
        u.rng_state = runtime.rng_advance(u.rng_state, u.rng_inc)
        return loss

    def evaluate(self, dataset, ema=False, **kw):
        """PSNR and SSIM of the network on a runtime.Dataset of held-out views (runtime.Testbed.evaluate: run.py's test loop, on the device; **kw goes there: spp,
        color_space, background, min_transmittance, stream).  The views are rendered with the trainer's live parameters, or with ema=True by a second NerfNetwork
        loaded from optimizer.export_fp16(OPT_EXPORT_EMA) with a copy of the live network's density grid as it is now.  Returns (summary, records).  Training state --
        parameters, optimiser, generator, counters -- is untouched: the next step computes what it computes without the evaluation.
        ema=True WAITS FOR THE DEVICE before it renders, which the live evaluation does not: the library takes a density grid from the host only, so the grid makes a
        round trip (10 M floats down and up, and the second network's bitfield is rebuilt), on every call -- the grid may have changed since the last one.  The export
        and the two uploads run on the current stream, which is drained before the first view is rendered, so a `stream` in **kw sees them complete.  With the live
        parameters a `stream` other than the current one is the caller's to order behind the training steps, as everywhere in this harness."""
        if self._eval_testbed is None:
            self._eval_testbed = runtime.Testbed(self.ctx, self.desc, network=self.network)
            self._eval_testbed.cone_angle_constant = self.cone_angle_constant
        net = self.network
        if ema:
            if self._ema_network is None:
                self._ema_network = runtime.NerfNetwork(self.ctx, self.desc, cell_cache_bytes=0)
            net = self._ema_network
            net.set_params_device(self.optimizer.export_fp16(_abi.OPT_EXPORT_EMA))
            net.set_density_grid(self.network.get_density_grid())
            torch.cuda.current_stream(f"cuda:{self.ctx.device}").synchronize()
        # the envmap as the testbed renders it: the EMA texels with ema=True, the live ones otherwise (params_inference() / params())
        self._eval_testbed.envmap = None if self.envmap is None else self.envmap.export(ema=bool(ema))
        return self._eval_testbed.evaluate(net, dataset, **kw)

    def fit(self, dataset, n_steps, n_rays=4096, grid_every=16, snap=True, random_bg=True, error_map=None):
        """Train on a runtime.Dataset for n_steps steps.  At training step 0 the cells no camera sees are marked untrained (mark_untrained_density_grid with
        clear_visible_voxels, src/testbed_nerf.cu:3452-3465) in front of the first grid update; the grid is updated every grid_every steps (the reference's cadence: 16).
        error_map: None, or an ErrorMapSchedule (step_dataset).  Returns the losses, 0-d CUDA tensors."""
        losses = []
        for _ in range(int(n_steps)):
            if self.training_step == 0:
                dataset.mark_untrained(self.network, clear_visible=True)
            if self.training_step % int(grid_every) == 0:
                self.update_density_grid()
            losses.append(self.step_dataset(dataset, n_rays, snap=snap, random_bg=random_bg, error_map=error_map))
        return losses
