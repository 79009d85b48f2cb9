#!/usr/bin/env python3
"""Times the training step and the side parameters' calls of two checkouts against each other on the GPU: a refactor's before and after.

    python tools/training_step_ab.py --a <checkout A, built> --b <checkout B, built> [--rounds 7] [--out result.json]

Every round starts one child process per side, A then B, so a drift of the machine falls on both alike; a child loads ITS checkout's package and library, and times
  - Trainer.step_dataset at 4096 rays on exposure_probe.py's dataset (8 images of 128 x 128) in four configurations -- plain, with an envmap, with an exposure, with
    both -- the four alternating batch by batch;
  - the calls alone, at envmap_train_probe.py's and exposure_probe.py's shapes for 4096 slots: Envmap.background / accumulate / accumulate + step on a 256 x 128
    map, Exposure.targets / accumulate / step on 100 images.
Times are device events around a batch of calls (probe_timing.py).  The result holds, per measurement and side, the median, minimum and maximum over all batches of all
rounds, and the difference of the two medians.  With --a and --b the same checkout that difference is the spread of the method itself: the margin for a comparison
made the same way.  No pass bar."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

N_RAYS, W, H, N_IMAGES, RES = 4096, 128, 128, 8, (256, 128)
DEV = "cuda:0"


def child(root, batches):
    sys.path.insert(0, os.path.abspath(root))
    import numpy as np
    import torch
    from nerfshop_amd import _abi, runtime, synth
    from nerfshop_amd.trainer import Trainer
    from probe_timing import timed
    ctx = runtime.Context(0)
    desc, grid = synth.model_desc(1), synth.density_grid(1)
    ds = runtime.Dataset(ctx, N_IMAGES, W, H)
    focal = 0.5 * W / math.tan(0.5 * synth.CAMERA_ANGLE_X)
    rng = np.random.default_rng(3)
    for k in range(N_IMAGES):
        img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
        img[..., 3] = 255
        ds.set_image(k, img)
        cam = _abi.TrainingCamera()
        cam.xform_start[:] = cam.xform_end[:] = synth.orbit_camera(360.0 * k / N_IMAGES).tolist()
        cam.focal_length[:], cam.principal_point[:] = (focal, focal), (0.5, 0.5)
        ds.set_camera(k, cam)
    configs = {"plain": {}, "envmap": dict(envmap=RES), "exposure": dict(exposure=True), "envmap and exposure": dict(envmap=RES, exposure=True)}
    trainers = {name: Trainer(ctx, desc, seed=11, density_grid=grid, max_samples=16 * N_RAYS, **kw) for name, kw in configs.items()}
    cand = {f"step_dataset, {name}": ((lambda t: lambda: t.step_dataset(ds, N_RAYS))(t), 16, None) for name, t in trainers.items()}

    # the calls alone: every slot live and depositing
    g = torch.Generator(device=DEV).manual_seed(7)
    env = runtime.Envmap(ctx, *RES)
    env.set_texels(np.random.default_rng(5).random((RES[1], RES[0], 4)).astype(np.float32))
    d = torch.randn((N_RAYS, 3), device=DEV, generator=g)
    sphere = torch.cat([torch.rand((N_RAYS, 3), device=DEV, generator=g), d / d.norm(dim=1, keepdim=True)], 1).contiguous()
    shuffled, in_order = torch.randperm(N_RAYS, device=DEV, generator=g).to(torch.int32), torch.arange(N_RAYS, dtype=torch.int32, device=DEV)
    counter = torch.tensor([N_RAYS], dtype=torch.int32, device=DEV)
    bg = torch.rand((N_RAYS, 3), device=DEV, generator=g)
    aux = (torch.rand((N_RAYS, _abi.RAY_AUX_WORDS), device=DEV, generator=g) - 0.3).view(torch.int32).clone()
    aux[:, 10:12] = 8
    numsteps_out = torch.full((N_RAYS, 2), 8, dtype=torch.int32, device=DEV)
    env_acc = _abi.EnvmapAccumulateParams(_abi.LOSS_L2, _abi.LOSS_RELATIVE_L2, 128.0, 0)
    env_out = env.background(sphere, shuffled, counter, background=bg)
    n_images = 100
    exp = runtime.Exposure(ctx, n_images)
    exp.set(np.random.default_rng(n_images).uniform(-1, 1, (n_images, 3)).astype(np.float32))
    runs = (torch.arange(N_RAYS, device=DEV) * n_images // N_RAYS).to(torch.int32)
    pixels = torch.stack([runs, torch.zeros_like(runs)], 1).contiguous()
    target = torch.rand((N_RAYS, 4), device=DEV, generator=g)
    exp_acc = _abi.ExposureAccumulateParams(128.0, 0)
    exp_out = exp.targets(in_order, counter, pixels, target)
    reset = lambda: exp.step(128.0, 0.0)   # (the handle counts the rays since its last step)
    cand.update({
        "Envmap.background": (lambda: env.background(sphere, shuffled, counter, background=bg, out=env_out), 50, None),
        "Envmap.accumulate": (lambda: env.accumulate(env_acc, counter, numsteps_out, aux, *env_out), 50, None),
        "Envmap.accumulate + step": (lambda: (env.accumulate(env_acc, counter, numsteps_out, aux, *env_out), env.step(128.0, 1e-2)), 50, None),
        "Exposure.targets": (lambda: exp.targets(in_order, counter, pixels, target, out=exp_out), 50, None),
        "Exposure.accumulate": (lambda: exp.accumulate(exp_acc, counter, in_order, numsteps_out, aux, exp_out[1]), 50, reset),
        "Exposure.step": (lambda: exp.step(128.0, 1e-2), 50, None)})
    for fn, calls, after in cand.values():
        timed(fn, max(calls // 4, 1), after)   # warm-up (the first dataset step makes the exposure)
    times = {name: [] for name in cand}
    for _ in range(batches):
        for name, (fn, calls, after) in cand.items():
            torch.cuda.synchronize()   # a batch starts on an idle device: a step is bound by its host work, and a backlog would hide that
            times[name].append(timed(fn, calls, after))
    torch.cuda.synchronize()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "times_us": times}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--a", help="a built checkout: side A")
    ap.add_argument("--b", help="a built checkout: side B")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batches", type=int, default=5, help="batches per measurement in one child")
    ap.add_argument("--out", default=None, help="write the JSON here")
    ap.add_argument("--child", default=None, help="(the child's mode) time this checkout and print the JSON")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.batches)
    sides = {"a": os.path.abspath(a.a), "b": os.path.abspath(a.b)}
    env = {k: v for k, v in os.environ.items() if k != "NRS_LIB_PATH"}   # each side loads its own library
    times, device = {side: {} for side in sides}, None
    for r in range(a.rounds):
        for side, root in sides.items():
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, "--batches", str(a.batches)], env=env, stdout=subprocess.PIPE, check=True,
                                 timeout=300)
            got = json.loads(out.stdout.decode().strip().splitlines()[-1])
            device = got["device"]
            for name, t in got["times_us"].items():
                times[side].setdefault(name, []).extend(t)
        print(f"round {r + 1} of {a.rounds} done", file=sys.stderr, flush=True)
    rows = {}
    for name in times["a"]:
        row = {side: {"median_us": statistics.median(times[side][name]), "min_us": min(times[side][name]), "max_us": max(times[side][name])} for side in sides}
        row["b_minus_a_us"] = row["b"]["median_us"] - row["a"]["median_us"]
        rows[name] = row
        print(f"{name}: a {row['a']['median_us']:.1f} us ({row['a']['min_us']:.1f} -- {row['a']['max_us']:.1f}), b {row['b']['median_us']:.1f} us "
              f"({row['b']['min_us']:.1f} -- {row['b']['max_us']:.1f}), b - a {row['b_minus_a_us']:+.1f} us", file=sys.stderr)
    result = {"device": device, "a": sides["a"], "b": sides["b"], "rounds": a.rounds, "batches": a.batches, "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
