"""The reference's training loop from the ray on, end to end on the device: samples -> inference -> ray loss -> backward -> the fused optimiser step.

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


class Trainer:
    """A NerfNetwork without cell records, an Optimizer bound to it, one persistent gradient buffer (zero between steps: the optimiser clears what it reads) and
    base.json's learning-rate schedule.

        trainer = Trainer(ctx, desc, seed=11, density_grid=synth.density_grid(1))
        losses = [trainer.step(rays, target_rgba) for _ in range(16)]          # 0-d CUDA tensors; float(losses[-1]) waits for the device
        trainer.update_density_grid()
    """

    def __init__(self, ctx, desc, seed=1337, weights=None, density_grid=None, max_samples=1 << 18, max_cascade=0, cone_angle_constant=0.0, adam=None,
                 loss_params=None, learning_rate=_abi.BASE_LEARNING_RATE, decay=(_abi.BASE_DECAY_START, _abi.BASE_DECAY_INTERVAL, _abi.BASE_DECAY_BASE),
                 density_grid_decay=0.95):
        self.ctx, self.lib, self.desc = ctx, ctx.lib, desc
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
        self._loss_bufs = None
        self._grid_update = _abi.GridUpdate()
        self._grid_update.max_cascade, self._grid_update.ema_step = int(max_cascade), 0
        self._grid_update.rng_state, self._grid_update.rng_inc = runtime.rng_seed(seed)
        self.density_grid_decay = float(density_grid_decay)
        self._grid_step = 0  # the training step of the last update_density_grid
        if density_grid is not None:
            self.network.set_density_grid(np.ascontiguousarray(density_grid, dtype=np.float32))
        else:
            self.update_density_grid()

    def current_learning_rate(self):
        start, interval, base = self.decay
        return runtime.exponential_decay_lr(self.training_step, self.learning_rate, start, interval, base)

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

    def step(self, rays, target_rgba, jitter=None, background=None):
        """One training step on rays [n, 6] f32 with the colours they should have, target_rgba [n, 4] f32 (linear, premultiplied); jitter [n] in [0, 1) or None,
        background [n, 3] (sRGB-encoded) or None for loss_params.background.  Returns the mean loss as a 0-d CUDA tensor.  Nothing waits for the device."""
        net = self.network
        n_rays = int(rays.shape[0])
        if tuple(target_rgba.shape) != (n_rays, 4):
            raise NrsError("Trainer.step: target_rgba must be [n_rays, 4]")
        coords, numsteps, ray_indices, counters = net.training_samples(None, rays, jitter, self.cone_angle_constant, self.max_samples)
        net.inference_strided(None, coords, self._out16)
        # the loss reads its per-ray inputs by ray SLOT: gather them with the generator's indices (slots at or past counters[0] are not live)
        slots = ray_indices.to(torch.int64)
        target = target_rgba.index_select(0, slots)
        bg = None if background is None else background.index_select(0, slots)
        if self._loss_bufs is None or self._loss_bufs[0].shape[0] != n_rays:
            self._loss_bufs = net.ray_loss_buffers(n_rays, self.max_samples, device=rays.device)
        _, coords_out, dl, loss, _ = net.ray_loss(None, self.loss_params, numsteps, coords, self._out16, target, background=bg, ray_counter=counters[:1],
                                                  out=self._loss_bufs)
        net.backward(None, coords_out, dl, self.grad, None, accumulate=True)
        self.optimizer.step(self.grad, loss_scale=float(self.loss_params.loss_scale), lr=self.current_learning_rate(), zero_grad=True)
        self.training_step += 1
        return loss.sum()

    def step_dataset(self, dataset, n_rays=4096, snap=True, random_bg=True):
        """One training step on n_rays pixels of a runtime.Dataset: dataset.rays (image and pixel selection, the pixel's camera, lens distortion; the target colour and
        the random background the loss composites behind it) -> step().  The generator is the trainer's m_rng (the one update_density_grid draws from), advanced once per
        step by NRS_RNG_STEP_DELTA as the reference advances it (src/testbed_nerf.cu:4435); n_rays_total counts the rays of the steps before.  snap and random_bg
        default to the reference's Testbed initialisers (include/neural-graphics-primitives/testbed.h:584 and :581).  Like step, nothing waits for the device."""
        u = self._grid_update
        rays, jitter, target, background, _ = dataset.rays(n_rays, self.n_rays_total, (u.rng_state, u.rng_inc), snap=snap, random_bg=random_bg, want_pixels=False)
        loss = self.step(rays, target, jitter=jitter, background=background)
        self.n_rays_total = (self.n_rays_total + int(n_rays)) & 0xffffffff
        u.rng_state = runtime.rng_advance(u.rng_state, u.rng_inc)
        return loss

    def fit(self, dataset, n_steps, n_rays=4096, grid_every=16, snap=True, random_bg=True):
        """Train on a runtime.Dataset for n_steps steps.  At training step 0 the cells no camera sees are marked untrained (mark_untrained_density_grid with
        clear_visible_voxels, src/testbed_nerf.cu:3452-3465) in front of the first grid update; the grid is updated every grid_every steps (the reference's cadence: 16).
        Returns the losses, 0-d CUDA tensors."""
        losses = []
        for _ in range(int(n_steps)):
            if self.training_step == 0:
                dataset.mark_untrained(self.network, clear_visible=True)
            if self.training_step % int(grid_every) == 0:
                self.update_density_grid()
            losses.append(self.step_dataset(dataset, n_rays, snap=snap, random_bg=random_bg))
        return losses
