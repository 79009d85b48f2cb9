#!/usr/bin/env python3
"""Times per-image exposure on the GPU and writes profiles/exposure_training.md.

    make -C nerfshop_amd/csrc variant NAME=exposure_nopeel VFLAGS=-DNRS_EXPOSURE_NO_PEEL      # the accumulate kernel with one atomic per lane: measurements only
    python tools/exposure_probe.py [--rounds 9] [--nopeel-lib nerfshop_amd/csrc/variants/libnrs_exposure_nopeel.so] [--md profiles/exposure_training.md]

1. nrs_exposure_accumulate at 4096 and 2^18 rays on 4 and 100 images, every slot live and depositing, slots in input order: images in runs of consecutive rays
   (what image_idx hands out) and, the peel's worst case, an image drawn at random per ray.  With --nopeel-lib the same in a child process that loads that library
   (NRS_LIB_PATH): what the peel buys.  nrs_exposure_targets beside it.
2. nrs_exposure_step at 100 and 4096 images.
3. Trainer.step_dataset at 4096 rays with and without an exposure, the two trainers alternating round by round.  Without an exposure no line of the step differs
   from the parent commit's, so that column is the parent's step.

Times are device events around a batch of calls (a caller's view: launches and host work included): median, minimum and maximum over the rounds.  No pass bar."""
import argparse
import json
import math
import os
import subprocess
import sys

import numpy as np
import torch

import probe_timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerfshop_amd import _abi, runtime, synth  # noqa: E402
from nerfshop_amd.trainer import Trainer  # noqa: E402

DEV = "cuda:0"
W, H, N_IMAGES = 128, 128, 8


def alternate(candidates, rounds, calls, title, after=None):
    return probe_timing.alternate(candidates, rounds, calls, title, after=after, file=sys.stderr)   # (stdout carries the JSON)


def kernels(ctx, rounds):
    """the accumulate and the targets kernel alone"""
    out = {}
    for n_rays, calls in ((4096, 50), (1 << 18, 8)):   # 8 x 2^18 = 2^21: the handle's ray count is reset behind every batch
        for n_images in (4, 100):
            exp = runtime.Exposure(ctx, n_images)
            exp.set(np.random.default_rng(n_images).uniform(-1, 1, (n_images, 3)).astype(np.float32))
            g = torch.Generator(device=DEV).manual_seed(7)
            ray_indices = torch.arange(n_rays, dtype=torch.int32, device=DEV)
            counter = torch.tensor([n_rays], dtype=torch.int32, device=DEV)
            aux = (torch.rand((n_rays, _abi.RAY_AUX_WORDS), device=DEV, generator=g) - 0.3).view(torch.int32).clone()
            numsteps_out = torch.full((n_rays, 2), 8, dtype=torch.int32, device=DEV)
            target = torch.rand((n_rays, 4), device=DEV, generator=g)
            acc = _abi.ExposureAccumulateParams(128.0, 0)
            runs = (torch.arange(n_rays, device=DEV) * n_images // n_rays).to(torch.int32)
            rand = torch.randint(0, n_images, (n_rays,), device=DEV, generator=g).to(torch.int32)
            pix = {name: torch.stack([img, torch.zeros_like(img)], 1).contiguous() for name, img in (("runs", runs), ("random", rand))}
            bufs = {name: exp.targets(ray_indices, counter, p, target) for name, p in pix.items()}
            cand = {"targets": lambda: exp.targets(ray_indices, counter, pix["runs"], target, out=bufs["runs"]),
                    "accumulate, images in runs": lambda: exp.accumulate(acc, counter, ray_indices, numsteps_out, aux, bufs["runs"][1]),
                    "accumulate, a random image per ray": lambda: exp.accumulate(acc, counter, ray_indices, numsteps_out, aux, bufs["random"][1])}
            out[f"{n_rays} rays, {n_images} images"] = alternate(cand, rounds, calls, f"{n_rays} rays, {n_images} images", after=lambda: exp.step(128.0, 0.0))
            torch.cuda.synchronize()
            exp.close()
    return out


def steps(ctx, rounds):
    out = {}
    for n_images in (100, 4096):
        exp = runtime.Exposure(ctx, n_images)
        out[f"{n_images} images"] = alternate({"step": lambda: exp.step(128.0, 1e-2)}, rounds, 50, f"nrs_exposure_step, {n_images} images")
        torch.cuda.synchronize()
        exp.close()
    return out


def dataset(ctx):
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
    return ds


def trainer_steps(ctx, rounds, n_rays=4096):
    desc, grid, ds = synth.model_desc(1), synth.density_grid(1), dataset(ctx)
    trainers = {"without an exposure (the parent's step)": Trainer(ctx, desc, seed=11, density_grid=grid, max_samples=16 * n_rays),
                "with an exposure": Trainer(ctx, desc, seed=11, density_grid=grid, max_samples=16 * n_rays, exposure=True)}
    cand = {name: (lambda t: lambda: t.step_dataset(ds, n_rays))(t) for name, t in trainers.items()}
    return alternate(cand, rounds, 16, f"Trainer.step_dataset, {n_rays} rays, {N_IMAGES} images")


def table(rows, header):
    lines = ["| " + " | ".join(header) + " |", "|" + "---|" * len(header)]
    lines += ["| " + " | ".join(r) + " |" for r in rows]
    return "\n".join(lines)


def cell(r):
    return f"{r['median_us']:.1f} ({r['min_us']:.1f} -- {r['max_us']:.1f})"


def markdown(result):
    k, nk = result["kernels"], result.get("kernels_nopeel")
    md = ["# Per-image exposure: what it costs", "",
          f"`tools/exposure_probe.py` on {result['device']}; microseconds per call between two device events, median (minimum -- maximum) over {result['rounds']} rounds.  "
          "Every slot is live and deposits; slots are in input order.", "", "## The accumulate kernel, with and without the peel", ""]
    rows = []
    for shape, r in k.items():
        for name in ("accumulate, images in runs", "accumulate, a random image per ray"):
            rows.append([shape, name.split(", ", 1)[1], cell(r[name]), cell(nk[shape][name]) if nk else "not measured"])
    md += [table(rows, ["batch", "images", "one atomic per image, channel and wave (the library)", "one atomic per lane and channel (`-DNRS_EXPOSURE_NO_PEEL`, probe build only)"]), ""]
    md += ["## The other two kernels", "", table([[shape, cell(r["targets"])] for shape, r in k.items()], ["batch", "nrs_exposure_targets"]), "",
           table([[shape, cell(r["step"])] for shape, r in result["steps"].items()], ["handle", "nrs_exposure_step"]), "",
           "## A training step", "", table([[name, cell(r)] for name, r in result["trainer"].items()], ["Trainer.step_dataset, 4096 rays, 8 images of 128 x 128", "us per step"]), ""]
    return "\n".join(md)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--nopeel-lib", default=None, help="a library built with -DNRS_EXPOSURE_NO_PEEL: its accumulate is timed in a child process")
    ap.add_argument("--kernels-only", action="store_true", help="(the child's mode) time the kernels and print the JSON")
    ap.add_argument("--md", default=None, help="write the tables here")
    ap.add_argument("--out", default=None, help="write the JSON here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exposure_probe: needs a GPU (there is nothing to measure without one)")
    ctx = runtime.Context(0)
    if a.kernels_only:
        print(json.dumps(kernels(ctx, a.rounds)))
        return
    result = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "kernels": kernels(ctx, a.rounds), "steps": steps(ctx, a.rounds)}
    result["trainer"] = trainer_steps(ctx, a.rounds)
    torch.cuda.synchronize()
    if a.nopeel_lib:
        env = dict(os.environ, NRS_LIB_PATH=os.path.abspath(a.nopeel_lib))
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernels-only", "--rounds", str(a.rounds)], env=env, stdout=subprocess.PIPE, check=True, timeout=600)
        result["kernels_nopeel"] = json.loads(child.stdout.decode().strip().splitlines()[-1])
    for path, text in ((a.out, json.dumps(result, indent=1)), (a.md, markdown(result))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
