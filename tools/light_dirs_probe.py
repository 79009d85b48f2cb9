"""What the light term costs: a 1080p frame of bench.py's lego scene with its cage edit, rendered by the plain model and by a model trained with light directions
(n_extra_dims = 3: the plain parameters with 16 more Xavier columns in the first rgb matrix, synth.make_light_params), on the same GPU in one process.

The two are timed interleaved (plain, light, plain, light ...) with HIP events around one frame, as bench.py times a frame; frames are cleared outside the timed region.
The light model runs the LIGHT twin of the default kernel: one more MFMA in layer 0 of the rgb network, 25 issues per 32-sample block instead of 24.
Prints the median and the 10th..90th percentile spread of the ms per frame and the Gsamples/s of both, and their ratio; --json adds one machine-readable line.

    python tools/light_dirs_probe.py [--reps 30] [--warmup 5] [--json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    import torch
    import bench
    from nerfshop_amd import runtime as rt, synth

    ctx = rt.Context(0)
    W, H = 1920, 1080
    scene = bench.build_scene("lego_cage", rt, synth, ctx, torch)
    tb = scene["tb"]
    desc = scene["desc"]
    light_tb = rt.Testbed(ctx, desc, scene["aabb_scale"], n_extra_dims=3)
    light_tb.nerf_network.set_params(synth.make_light_params(desc, sigma_raw=synth.default_sigma_raw(scene["aabb_scale"])))
    light_tb.nerf_network.set_density_grid(scene["grid"])
    light_tb.edit_operators = list(tb.edit_operators)
    p = synth.render_params(W, H, bench.camera_for(2, synth, scene["aabb_scale"]), aabb_scale=scene["aabb_scale"], apply_operators=True)
    frame = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    depth = torch.zeros((H, W), dtype=torch.float32, device="cuda:0")
    rigs = {"plain": tb, "light": light_tb}
    samples = {}
    for name, t in rigs.items():
        frame.zero_()
        samples[name] = int(t.render_with_params(t.nerf_network, p, frame, depth, None, None, want_stats=True).n_samples)
    assert samples["plain"] == samples["light"], "the density network is the same: both march the same samples"
    ms = {"plain": [], "light": []}
    for rep in range(args.warmup + args.reps):
        for name, t in rigs.items():
            frame.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t.render_with_params(t.nerf_network, p, frame, depth, None, None, False)
            e1.record()
            torch.cuda.synchronize()
            if rep >= args.warmup:
                ms[name].append(e0.elapsed_time(e1))
    row = {"workload": "lego_cage", "width": W, "height": H, "samples_per_frame": samples["plain"]}
    for name in rigs:
        v = np.asarray(ms[name])
        row[name] = {"ms_per_frame": round(float(np.median(v)), 4), "p10": round(float(np.quantile(v, 0.1)), 4), "p90": round(float(np.quantile(v, 0.9)), 4),
                     "gsamples_per_s": round(samples[name] / float(np.median(v)) / 1e6, 3)}
        print(f"{name:5s} {W}x{H}: {row[name]['ms_per_frame']:.4f} ms/frame [{row[name]['p10']:.4f} .. {row[name]['p90']:.4f}] {row[name]['gsamples_per_s']:.2f} Gsamples/s", flush=True)
    row["light_over_plain"] = round(row["light"]["ms_per_frame"] / row["plain"]["ms_per_frame"], 4)
    print(f"light / plain = {row['light_over_plain']:.4f} (one MFMA in 25 would be 1.04 of the MLP, less of the frame)")
    if args.json:
        print(json.dumps({"light_dirs_probe": row, "device": ctx.device_name}))


if __name__ == "__main__":
    main()
