#!/usr/bin/env python3
"""Times the training error map's kernels on the GPU, in one process.

    python tools/error_map_probe.py [--parent path/to/the/parent/commit's/libnrs.so] [--out profiles/error_map_probe.json]

1. The ray kernel at 2^21 rays over 100 images of 256 x 256 with a 29 x 29 error map, the candidates alternating round by round as tools/dataset_rays_probe.py does:
   nrs_dataset_rays of --parent (when given) and of the tree, nrs_dataset_rays_ex with both switches off (without and with the xy / pdf outputs), with the pixel
   switch, the image switch and both.  Before anything is timed the outputs nrs_dataset_rays_ex shares with nrs_dataset_rays are compared with it, bit for bit.
2. nrs_dataset_error_map_accumulate at 2^21 slots, every ray live: on the rays of part 1 with both switches off (spread evenly) and with both on (crowded into the
   map's heavy cells).
3. nrs_dataset_error_map_build_cdfs at 100 and at 1025 images of 29 x 29 cells, and at 100 images of 256 x 256 cells.

Times are device events around a batch of launches: median, minimum and maximum over the rounds.  No pass bar: the numbers go into profiles/error_map.md."""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import torch

import probe_timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerfshop_amd import _abi, runtime, synth  # noqa: E402

N_RAYS, N_IMAGES, RES, MAP_RES = 1 << 21, 100, 256, 29
DEV = "cuda:0"


def bind_parent(path):
    """the parent's library with the prototypes this probe uses"""
    lib = C.CDLL(path)
    P, U32, I = C.c_void_p, C.c_uint32, C.c_int
    lib.nrs_last_error.restype = C.c_char_p
    lib.nrs_ctx_create.argtypes = [I, C.POINTER(P)]
    lib.nrs_dataset_create.argtypes = [P, U32, U32, U32, C.POINTER(P)]
    lib.nrs_dataset_set_image.argtypes = [P, U32, I, P, I, U32, U32, P]
    lib.nrs_dataset_set_camera.argtypes = [P, U32, C.POINTER(_abi.TrainingCamera)]
    lib.nrs_dataset_rays.argtypes = [P, P, C.POINTER(_abi.DatasetRaysParams), U32, P, P, P, P, P]
    return lib


def cameras():
    cams = []
    focal = 0.5 * RES / math.tan(0.5 * synth.CAMERA_ANGLE_X)
    for k in range(N_IMAGES):
        cam = _abi.TrainingCamera()
        cam.xform_start[:] = synth.orbit_camera(360.0 * k / N_IMAGES).tolist()
        cam.xform_end[:] = synth.orbit_camera(360.0 * k / N_IMAGES + 2.0).tolist()
        cam.focal_length[:], cam.principal_point[:], cam.rolling_shutter[:] = (focal, focal * 1.01), (0.49, 0.52), (0.0, 0.3, 0.5, 0.2)
        cams.append(cam)
    return cams


def check(lib, status):
    if status != 0:
        raise RuntimeError(lib.nrs_last_error().decode())


def fill(lib, ctx_out, images, cams):
    ds = C.c_void_p()
    check(lib, lib.nrs_dataset_create(ctx_out, N_IMAGES, RES, RES, C.byref(ds)))
    for k in range(N_IMAGES):
        check(lib, lib.nrs_dataset_set_image(ds, k, _abi.IMAGE_RGBA16F_LINEAR, images[k].data_ptr(), 1, 0, 0, None))
        check(lib, lib.nrs_dataset_set_camera(ds, k, C.byref(cams[k])))
    return ds


def alternate(candidates, rounds, launches, title):
    return probe_timing.alternate(candidates, rounds, launches, title, warmup=launches)   # (a whole batch to warm up)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", default=None, help="libnrs.so of the parent commit: its nrs_dataset_rays joins the alternation")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("error_map_probe: needs a GPU (there is nothing to measure without one)")
    lib = _abi.load()
    ctx = runtime.Context(0)
    images = [torch.rand((RES, RES, 4), device=DEV).to(torch.float16) for _ in range(N_IMAGES)]
    cams = cameras()
    ds = fill(lib, ctx.h, images, cams)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = runtime.rng_seed(1337)

    def buffers():
        return [torch.zeros(N_RAYS * w, dtype=torch.float32, device=DEV) for w in (6, 1, 4, 3, 2)]
    plain_p = _abi.DatasetRaysParams()
    plain_p.rng_state, plain_p.rng_inc, plain_p.n_rays_total, plain_p.snap_to_pixel_centers, plain_p.random_bg_color = rng[0], rng[1], 4096, 1, 1
    out_plain, out_ex = buffers(), buffers()
    xy, pdf = torch.zeros(N_RAYS * 2, dtype=torch.float32, device=DEV), torch.zeros(N_RAYS, dtype=torch.float32, device=DEV)

    def ex_params(by_images, by_pixels):
        p = _abi.DatasetRaysExParams()
        p.rng_state, p.rng_inc, p.n_rays_total, p.snap_to_pixel_centers, p.random_bg_color = rng[0], rng[1], 4096, 1, 1
        p.sample_images_by_error, p.sample_pixels_by_error = int(by_images), int(by_pixels)
        return p

    def plain(which_lib, which_ds, out):
        return lambda: check(which_lib, which_lib.nrs_dataset_rays(which_ds, stream(), C.byref(plain_p), N_RAYS, *[t.data_ptr() for t in out]))

    def ex(p, with_outputs):
        extra = (xy.data_ptr(), pdf.data_ptr()) if with_outputs else (None, None)
        return lambda: check(lib, lib.nrs_dataset_rays_ex(ds, stream(), C.byref(p), N_RAYS, *[t.data_ptr() for t in out_ex], *extra))

    # a heavy-tailed map, its CDFs
    data = (np.random.default_rng(5).pareto(0.7, (N_IMAGES, MAP_RES, MAP_RES)) * 1e-4).astype(np.float32)
    check(lib, lib.nrs_dataset_error_map_set(ds, MAP_RES, MAP_RES, data.ctypes.data))
    check(lib, lib.nrs_dataset_error_map_build_cdfs(ds, None))
    # flags off against the plain call, bit for bit
    plain(lib, ds, out_plain)()
    ex(ex_params(False, False), True)()
    torch.cuda.synchronize()
    for x, y in zip(out_plain, out_ex):
        if not torch.equal(x.view(torch.int32), y.view(torch.int32)):
            raise RuntimeError("nrs_dataset_rays_ex with both switches off differs from nrs_dataset_rays")
    if not bool((pdf == 1).all()):
        raise RuntimeError("the pdf is not 1 with both switches off")

    candidates = {}
    if a.parent:
        parent = bind_parent(a.parent)
        pctx = C.c_void_p()
        check(parent, parent.nrs_ctx_create(0, C.byref(pctx)))
        pds = fill(parent, pctx, images, cams)
        out_parent = buffers()
        candidates["parent nrs_dataset_rays"] = plain(parent, pds, out_parent)
        candidates["parent nrs_dataset_rays"]()
        torch.cuda.synchronize()
        for x, y in zip(out_plain, out_parent):
            if not torch.equal(x.view(torch.int32), y.view(torch.int32)):
                raise RuntimeError("nrs_dataset_rays differs from the parent's")
    candidates["nrs_dataset_rays"] = plain(lib, ds, out_plain)
    candidates["rays_ex off, no xy / pdf"] = ex(ex_params(False, False), False)
    candidates["rays_ex off"] = ex(ex_params(False, False), True)
    candidates["rays_ex pixels"] = ex(ex_params(False, True), True)
    candidates["rays_ex images"] = ex(ex_params(True, False), True)
    candidates["rays_ex images + pixels"] = ex(ex_params(True, True), True)
    result = {"device": torch.cuda.get_device_name(0), "rays": alternate(candidates, a.rounds, a.launches, f"{N_RAYS} rays, {N_IMAGES} images, map {MAP_RES} x {MAP_RES}")}

    # accumulate: every slot live; the rays of both switches off (spread evenly over the cells) and of both on (crowded into the heavy cells: the same few
    # addresses take most of the atomics)
    counter = torch.tensor([N_RAYS], dtype=torch.int32, device=DEV)
    ray_indices = torch.randperm(N_RAYS, device=DEV).to(torch.int32)
    loss = (torch.rand(N_RAYS, device=DEV) * (0.3 / N_RAYS)).contiguous()
    accs = {}
    for name, key in (("uniform rays", "rays_ex off"), ("rays drawn from the CDFs", "rays_ex images + pixels")):
        candidates[key]()
        torch.cuda.synchronize()
        held = (out_ex[4].clone(), xy.clone(), pdf.clone())
        accs[name] = (lambda h: lambda: check(lib, lib.nrs_dataset_error_map_accumulate(ds, stream(), N_RAYS, counter.data_ptr(), ray_indices.data_ptr(), loss.data_ptr(),
                                                                                       h[1].data_ptr(), h[0].data_ptr(), h[2].data_ptr(), None)))(held)
    check(lib, lib.nrs_dataset_error_map_reset(ds, MAP_RES, MAP_RES, None))
    result["accumulate"] = alternate(accs, a.rounds, a.launches, f"accumulate, {N_RAYS} slots, map {MAP_RES} x {MAP_RES}")

    # build_cdfs
    result["build_cdfs"] = {}
    for n_images, res in ((100, MAP_RES), (1025, MAP_RES), (100, 256)):
        d = runtime.Dataset(ctx, n_images, res, res)
        d.error_map_set((np.random.default_rng(n_images).pareto(0.7, (n_images, res, res)) * 1e-4).astype(np.float32))
        build = lambda: check(lib, lib.nrs_dataset_error_map_build_cdfs(d.h, stream()))
        result["build_cdfs"][f"{n_images} images, {res} x {res}"] = alternate({"build_cdfs": build}, a.rounds, a.launches, f"{n_images} images, map {res} x {res}")["build_cdfs"]
        torch.cuda.synchronize()
        d.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
