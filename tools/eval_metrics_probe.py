#!/usr/bin/env python3
"""Times the image metrics on the GPU, in one process.

    python tools/eval_metrics_probe.py [--out profiles/eval_metrics_probe.json] [--views 4] [--eval-res 400]

1. nrs_image_metrics (the clear, image_metrics_kernel, the one-thread finish kernel) at 800 x 800 and 1920 x 1080 with an fp16 reference in the Linear colour space,
   with and without the two maps, and with the sRGB blend, alternating round by round with nrs_tonemap on the same buffer (RGBA32F output, sRGB): a pure streaming
   pass over the same image and the yardstick.  Reported: microseconds per call, the ratio to the tonemap, and the bytes per pixel each MUST move (image 16 + reference 8
   [+ 8 for the maps] against the tonemap's 16 + 16) and the rate that gives -- not a counter reading.
2. Testbed.evaluate per view at --eval-res squared and 8 spp against the path it replaces: render_to_cpu (linear) of the same view plus tests/metrics_ref.py on
   the host.  Both include the rendering; the difference is the read-back and the host arithmetic.  The records of the two paths are compared before anything is timed.

Times are device events around a batch of launches (part 1) and a host clock around work that ends in a synchronisation (part 2): median, minimum and maximum over
the rounds.  No pass bar: the numbers go into profiles/eval_metrics.md."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from nerfshop_amd import _abi, runtime, synth  # noqa: E402
from nerfshop_amd.runtime import metrics  # noqa: E402
import metrics_ref  # noqa: E402

DEV = "cuda:0"
ROUNDS, BATCH = 15, 50


def stats(us):
    return {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us)}


def time_batches(candidates):
    """candidates: name -> callable that enqueues one call.  Round-robin over the candidates, ROUNDS rounds of BATCH calls each, device events around a batch."""
    for fn in candidates.values():
        for _ in range(BATCH):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in candidates}
    for _ in range(ROUNDS):
        for name, fn in candidates.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(BATCH):
                fn()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) * 1000.0 / BATCH)
    return {k: stats(v) for k, v in out.items()}


def kernel_part(ctx, width, height):
    g = torch.Generator(device=DEV).manual_seed(width)
    image = torch.rand((height, width, 4), generator=g, device=DEV, dtype=torch.float32) * 1.2 - 0.1
    reference = (image * 0.97 + 0.01).to(torch.float16)
    reference[..., 3] = 1.0
    rec = torch.zeros(32, dtype=torch.uint8, device=DEV)
    maps = torch.empty((2, height, width), dtype=torch.float32, device=DEV)
    out = torch.empty_like(image)
    lib, stream = ctx.lib, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p_lin, p_srgb = metrics.metrics_params(0), metrics.metrics_params(1)
    t = _abi.TonemapParams()
    t.background_color[:] = (0.0, 0.0, 0.0, 1.0)
    t.output_color_space, t.output_format = 1, _abi.TONEMAP_RGBA32F

    def run_metrics(p, with_maps):
        m0, m1 = (maps[0].data_ptr(), maps[1].data_ptr()) if with_maps else (None, None)
        return lambda: _abi.check(lib.nrs_image_metrics(ctx.h, stream, width, height, image.data_ptr(), reference.data_ptr(), C.byref(p), rec.data_ptr(), m0, m1))
    # what is timed computes what the twin computes
    run_metrics(p_lin, True)()
    torch.cuda.synchronize()
    got = metrics.records_from_bytes(rec)[0]
    want = runtime.image_metrics_host(image.cpu().numpy(), reference.cpu().numpy())[0]
    agree = {"ssim_diff": abs(float(got["ssim"]) - float(want["ssim"])), "mse_rel": abs(float(got["mse"]) - float(want["mse"])) / float(want["mse"])}
    assert agree["ssim_diff"] <= 2e-5 and agree["mse_rel"] <= 1e-5, agree
    res = time_batches({
        "tonemap": lambda: _abi.check(lib.nrs_tonemap(ctx.h, stream, width, height, image.data_ptr(), C.byref(t), out.data_ptr())),
        "metrics": run_metrics(p_lin, False),
        "metrics_maps": run_metrics(p_lin, True),
        "metrics_srgb_blend": run_metrics(p_srgb, False),
    })
    n = width * height
    bytes_per_pixel = {"tonemap": 32, "metrics": 24, "metrics_maps": 32, "metrics_srgb_blend": 24}
    for k, v in res.items():
        v["bytes_per_pixel_needed"] = bytes_per_pixel[k]
        v["GB_per_s_of_needed_bytes"] = bytes_per_pixel[k] * n / v["median_us"] * 1e-3
        v["ratio_to_tonemap"] = v["median_us"] / res["tonemap"]["median_us"]
    return {"width": width, "height": height, "agreement_with_the_twin": agree, "calls": res}


def evaluate_part(ctx, n_views, res):
    desc = synth.model_desc(1)
    tb = runtime.Testbed(ctx, desc, 1)
    tb.nerf_network.set_params(synth.make_params(desc))
    tb.nerf_network.set_density_bitfield(synth.grid_to_bitfield(synth.density_grid(1)))
    focal = 0.5 * res / math.tan(0.5 * synth.CAMERA_ANGLE_X)
    black = (0.0, 0.0, 0.0, 1.0)
    ds = runtime.Dataset(ctx, n_views, res, res)
    cams = [synth.orbit_camera(360.0 * k / n_views + 15.0) for k in range(n_views)]
    tb.rendering_min_transmittance = 1e-4
    for k, cam in enumerate(cams):
        ds.set_image(k, tb.render_to_cpu(tb.nerf_network, res, res, 8, False, (focal, focal), cam, background=black, fmt="rgba8", apply_operators=False))
        c = _abi.TrainingCamera()
        c.xform_start[:] = c.xform_end[:] = cam.tolist()
        c.focal_length[:], c.principal_point[:] = (focal, focal), (0.5, 0.5)
        ds.set_camera(k, c)
    stored = [ds.get_image(k).astype(np.float32) for k in range(n_views)]

    def device_path():
        return tb.evaluate(tb.nerf_network, ds, spp=8)[1]

    def host_path():
        out = []
        for k, cam in enumerate(cams):
            frame = tb.render_to_cpu(tb.nerf_network, res, res, 8, True, (focal, focal), cam, background=black, apply_operators=False)
            out.append(metrics_ref.metrics(frame, stored[k]))
        return out
    dev, host = device_path(), host_path()
    agree = max(abs(float(dev["ssim"][k]) - float(host[k]["ssim"])) for k in range(n_views))
    assert agree <= 2e-5, agree
    times = {"evaluate": [], "render_to_cpu_plus_host_metrics": []}
    for _ in range(5):
        for name, fn in (("evaluate", device_path), ("render_to_cpu_plus_host_metrics", host_path)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e6 / n_views)
    out = {k: stats(v) for k, v in times.items()}
    return {"resolution": res, "views": n_views, "spp": 8, "psnr_mean": float(np.mean(dev["psnr"])), "max_ssim_difference_between_the_paths": agree, "per_view": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--eval-res", type=int, default=400)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_metrics_probe: needs a GPU (there is nothing to time without one)")
    ctx = runtime.Context(0)
    result = {"device": ctx.device_name, "kernel": [kernel_part(ctx, 800, 800), kernel_part(ctx, 1920, 1080)], "evaluate": evaluate_part(ctx, args.views, args.eval_res)}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
