#!/usr/bin/env python3
"""Times the dataset's ray kernel and a whole training step from a dataset, on the GPU, in one process.

    python tools/dataset_rays_probe.py [--variant NAME=path/to/libnrs_NAME.so ...] [--out profiles/dataset_rays_probe.json]

1. dataset_rays_kernel at 2^18 rays (a launch of that size is about as long as enqueueing it takes, so the figure is a launch rate as much as a kernel time) and at
   2^21 rays (the generator's limit: the kernel dominates) over 50 images of 256 x 256, for the library in the tree and for every --variant (an A/B build of nrs_dataset.hip: see
   profiles/dataset_rays.md for the ones that were measured), alternating between them round by round; pinhole cameras and cameras with the iterative lens model.
   Every variant's outputs are compared with the tree's, bit for bit, before anything is timed.
2. Trainer.step_dataset against Trainer.step on the very same rays, targets, jitter and backgrounds (taken from one dataset.rays call): what the dataset adds to a step.

Times are device events around a batch of launches, median and minimum over the rounds.  No pass bar: the numbers go into profiles/dataset_rays.md."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

import torch

import probe_timing
from probe_timing import alternate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerfshop_amd import _abi, runtime, synth  # noqa: E402
from nerfshop_amd.trainer import Trainer  # noqa: E402

RAY_COUNTS, N_IMAGES, RES = (1 << 18, 1 << 21), 50, 256
N_MAX = max(RAY_COUNTS)
DEV = "cuda:0"


def bind(path):
    """a second copy of the library with the prototypes this probe uses"""
    lib = C.CDLL(path)
    P, U32, I = C.c_void_p, C.c_uint32, C.c_int
    lib.nrs_last_error.restype = C.c_char_p
    lib.nrs_ctx_create.argtypes = [I, C.POINTER(P)]
    lib.nrs_dataset_create.argtypes = [P, U32, U32, U32, C.POINTER(P)]
    lib.nrs_dataset_set_image.argtypes = [P, U32, I, P, I, U32, U32, P]
    lib.nrs_dataset_set_camera.argtypes = [P, U32, C.POINTER(_abi.TrainingCamera)]
    lib.nrs_dataset_rays.argtypes = [P, P, C.POINTER(_abi.DatasetRaysParams), U32, P, P, P, P, P]
    lib.nrs_rng_seed.argtypes = [C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.nrs_rng_seed.restype = None
    return lib


def cameras(lens):
    cams = []
    focal = 0.5 * RES / math.tan(0.5 * synth.CAMERA_ANGLE_X)
    for k in range(N_IMAGES):
        cam = _abi.TrainingCamera()
        cam.xform_start[:] = synth.orbit_camera(360.0 * k / N_IMAGES).tolist()
        cam.xform_end[:] = synth.orbit_camera(360.0 * k / N_IMAGES + 2.0).tolist()
        cam.focal_length[:], cam.principal_point[:], cam.rolling_shutter[:] = (focal, focal * 1.01), (0.49, 0.52), (0.0, 0.3, 0.5, 0.2)
        if lens:
            cam.distortion_mode = 1
            cam.distortion_params[:4] = (0.0578421, -0.0805099, -0.000980296, 0.00015575)   # the fox dataset's
        cams.append(cam)
    return cams


class Rig:
    """one library's dataset and output buffers"""

    def __init__(self, name, lib, images, cams):
        self.name, self.lib = name, lib
        self.ctx, self.ds = C.c_void_p(), C.c_void_p()
        self.check(lib.nrs_ctx_create(0, C.byref(self.ctx)))
        self.check(lib.nrs_dataset_create(self.ctx, N_IMAGES, RES, RES, C.byref(self.ds)))
        for k in range(N_IMAGES):
            self.check(lib.nrs_dataset_set_image(self.ds, k, _abi.IMAGE_RGBA16F_LINEAR, images[k].data_ptr(), 1, 0, 0, None))
            self.check(lib.nrs_dataset_set_camera(self.ds, k, C.byref(cams[k])))
        self.out = [torch.zeros(N_MAX * w, dtype=torch.float32, device=DEV) for w in (6, 1, 4, 3, 2)]
        self.p = _abi.DatasetRaysParams()
        st, inc = C.c_uint64(), C.c_uint64()
        lib.nrs_rng_seed(1337, C.byref(st), C.byref(inc))
        self.p.rng_state, self.p.rng_inc, self.p.n_rays_total, self.p.snap_to_pixel_centers, self.p.random_bg_color = st.value, inc.value, 4096, 1, 1

    def check(self, status):
        if status != 0:
            raise RuntimeError(f"{self.name}: {self.lib.nrs_last_error().decode()}")

    def launch(self, n_rays):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.check(self.lib.nrs_dataset_rays(self.ds, stream, C.byref(self.p), n_rays, *[t.data_ptr() for t in self.out]))


def kernel_ab(libs, rounds, launches):
    images = [torch.rand((RES, RES, 4), device=DEV).to(torch.float16) for _ in range(N_IMAGES)]
    results = {}
    for lens in (False, True):
        cams = cameras(lens)
        rigs = [Rig(name, lib, images, cams) for name, lib in libs]
        for r in rigs:
            r.launch(N_MAX)
        torch.cuda.synchronize()
        for r in rigs[1:]:
            for a, b in zip(rigs[0].out, r.out):
                if not torch.equal(a.view(torch.int32), b.view(torch.int32)):
                    raise RuntimeError(f"{r.name}: outputs differ from {rigs[0].name}'s")
        for n_rays in RAY_COUNTS:
            key = f"{'iterative lens' if lens else 'pinhole'}, {n_rays} rays"
            candidates = {r.name: (lambda r: lambda: r.launch(n_rays))(r) for r in rigs}
            results[key] = alternate(candidates, rounds, launches, f"dataset_rays_kernel, {key}", warmup=launches)
    return results


def step_ab(rounds, steps, n_rays):
    ctx = runtime.Context(0)
    desc = synth.model_desc(log2_hashmap_size=14)
    W = H = 64
    tb = runtime.Testbed(ctx, desc, 1)
    tb.nerf_network.set_params(synth.make_params(desc))
    grid = synth.density_grid(1)
    tb.nerf_network.set_density_grid(grid)
    buf = runtime.RenderBuffer(W, H)
    ds = runtime.Dataset(ctx, 8, W, H)
    focal = 0.5 * W / math.tan(0.5 * synth.CAMERA_ANGLE_X)
    for k in range(8):
        camera = synth.orbit_camera(45.0 * k)
        p = synth.render_params(W, H, camera)
        p.linear_colors = 1
        buf.clear_frame()
        tb.render_with_params(tb.nerf_network, p, buf.frame_buffer(), buf.depth_buffer())
        ds.set_image(k, buf.frame_buffer().clone())
        cam = _abi.TrainingCamera()
        cam.xform_start[:] = cam.xform_end[:] = camera.tolist()
        cam.focal_length[:], cam.principal_point[:] = (focal, focal), (0.5, 0.5)
        ds.set_camera(k, cam)
    trainer = Trainer(ctx, desc, seed=11, density_grid=grid, max_samples=1 << 20)
    u = trainer._grid_update
    rays, jitter, target, background, pixels = ds.rays(n_rays, 0, (u.rng_state, u.rng_inc))

    def timed(fn):
        return probe_timing.timed(fn, steps) * 1e-3   # milliseconds per step

    with_dataset = lambda: trainer.step_dataset(ds, n_rays)
    on_rays = lambda: trainer.step(rays, target, jitter=jitter, background=background)
    timed(with_dataset), timed(on_rays)   # warm-up
    times = {"step_dataset": [], "step on the same rays": []}
    for _ in range(rounds):
        times["step_dataset"].append(timed(with_dataset))
        times["step on the same rays"].append(timed(on_rays))
    for name, t in times.items():
        print(f"Trainer, {n_rays} rays, {name}: median {statistics.median(t):.3f} ms per step, min {min(t):.3f}, max {max(t):.3f} over {rounds} rounds of {steps}")
    return {name: {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)} for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--variant", action="append", default=[], help="NAME=path of an A/B build of the library")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--step-rays", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dataset_rays_probe: needs a GPU (there is nothing to measure without one)")
    libs = [("tree", bind(_abi.LIB_PATH))] + [(v.split("=", 1)[0], bind(v.split("=", 1)[1])) for v in a.variant]
    result = {"device": torch.cuda.get_device_name(0), "kernel": kernel_ab(libs, a.rounds, a.launches), "step": step_ab(a.rounds, a.steps, a.step_rays)}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
