#!/usr/bin/env python3
"""Times training with an environment map on the GPU, in one process.

    python tools/envmap_train_probe.py [--rounds 9] [--out profiles/envmap_train_probe.json]

1. Trainer.step at 4096 and at 2^18 rays (max_samples 16 per ray), on fixed rays of a synthetic dataset, without an envmap -- the parent commit's code path: no line
   of it changed -- and with one of 256 x 128, the two trainers alternating round by round.  A round is a batch of steps between two device events, so the figure
   is what a caller sees per step, launches and host work included.
2. The three new kernels alone at both ray counts, every slot live and depositing, rays spread over the sphere: nrs_envmap_background, nrs_envmap_accumulate,
   nrs_envmap_step (cells -> gradient, then the optimiser's step on 4 x 256 x 128 floats).
3. nrs_envmap_accumulate with every ray aimed at ONE texel footprint: twelve cells take every atomic -- the worst contention.

Times are device events around a batch of calls: median, minimum and maximum over the rounds.  No pass bar: the numbers go into profiles/envmap_training.md."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

from probe_timing import alternate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerfshop_amd import _abi, runtime, synth  # noqa: E402
from nerfshop_amd.trainer import Trainer  # noqa: E402

DEV = "cuda:0"
RES = (256, 128)
W, H, N_IMAGES = 128, 128, 8


def dataset(ctx):
    ds = runtime.Dataset(ctx, N_IMAGES, W, H)
    focal = 0.5 * W / math.tan(0.5 * synth.CAMERA_ANGLE_X)
    rng = np.random.default_rng(3)
    for k in range(N_IMAGES):
        img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
        img[..., 3] = np.where(rng.random((H, W)) < 0.5, 255, 0)   # half of the pixels see the background
        ds.set_image(k, img)
        cam = _abi.TrainingCamera()
        cam.xform_start[:] = cam.xform_end[:] = synth.orbit_camera(360.0 * k / N_IMAGES).tolist()
        cam.focal_length[:], cam.principal_point[:] = (focal, focal), (0.5, 0.5)
        ds.set_camera(k, cam)
    return ds


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("envmap_train_probe: needs a GPU (there is nothing to measure without one)")
    ctx = runtime.Context(0)
    desc = synth.model_desc(1)
    grid = synth.density_grid(1)
    ds = dataset(ctx)
    result = {"device": torch.cuda.get_device_name(0), "envmap": list(RES), "steps": {}, "kernels": {}}
    for n_rays, calls in ((4096, 20), (1 << 18, 5)):
        trainers = {"without an envmap": Trainer(ctx, desc, seed=11, density_grid=grid, max_samples=16 * n_rays),
                    "with an envmap": Trainer(ctx, desc, seed=11, density_grid=grid, max_samples=16 * n_rays, envmap=RES)}
        rays, jitter, target, background, _ = ds.rays(n_rays, 0, runtime.rng_seed(1337), snap=True, random_bg=True, want_pixels=False)
        steps = {name: (lambda t: lambda: t.step(rays, target, jitter=jitter, background=background))(t) for name, t in trainers.items()}
        result["steps"][str(n_rays)] = alternate(steps, a.rounds, calls, f"Trainer.step, {n_rays} rays")
        torch.cuda.synchronize()
        del trainers, steps

        # the kernels alone: every slot live and depositing
        env = runtime.Envmap(ctx, *RES)
        env.set_texels(np.random.default_rng(5).random((RES[1], RES[0], 4)).astype(np.float32))
        g = torch.Generator(device=DEV).manual_seed(7)
        d = torch.randn((n_rays, 3), device=DEV, generator=g)
        d = d / d.norm(dim=1, keepdim=True)
        sphere = torch.cat([torch.rand((n_rays, 3), device=DEV, generator=g), d], 1).contiguous()
        one = sphere.clone()
        one[:, 3:] = torch.tensor([0.48, 0.6, 0.64], device=DEV)
        ray_indices = torch.randperm(n_rays, device=DEV, generator=g).to(torch.int32)
        counter = torch.tensor([n_rays], dtype=torch.int32, device=DEV)
        bg = torch.rand((n_rays, 3), device=DEV, generator=g)
        aux_f = torch.rand((n_rays, _abi.RAY_AUX_WORDS), device=DEV, generator=g) - 0.3   # g, T, target, C: values of the sizes a step has
        aux = aux_f.view(torch.int32).clone()
        aux[:, 10:12] = 8
        numsteps_out = torch.zeros((n_rays, 2), dtype=torch.int32, device=DEV)
        numsteps_out[:, 0] = 8
        acc = _abi.EnvmapAccumulateParams(_abi.LOSS_L2, _abi.LOSS_RELATIVE_L2, 128.0, 0)
        outs = {name: env.background(r, ray_indices, counter, background=bg) for name, r in (("sphere", sphere), ("one texel", one))}
        torch.cuda.synchronize()
        assert len(torch.unique(outs["one texel"][1], dim=0)) == 1
        kernels = {"background": lambda: env.background(sphere, ray_indices, counter, background=bg, out=outs["sphere"]),
                   "accumulate, rays over the sphere": lambda: env.accumulate(acc, counter, numsteps_out, aux, *outs["sphere"]),
                   "accumulate, every ray on one texel": lambda: env.accumulate(acc, counter, numsteps_out, aux, *outs["one texel"]),
                   "step (after an accumulate over the sphere)": lambda: (env.accumulate(acc, counter, numsteps_out, aux, *outs["sphere"]), env.step(128.0, 1e-2))}
        r = alternate(kernels, a.rounds, 50, f"{n_rays} slots, envmap {RES[0]} x {RES[1]}")
        r["step alone (difference)"] = {"median_us": r["step (after an accumulate over the sphere)"]["median_us"] - r["accumulate, rays over the sphere"]["median_us"]}
        result["kernels"][str(n_rays)] = r
        torch.cuda.synchronize()
        env.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
