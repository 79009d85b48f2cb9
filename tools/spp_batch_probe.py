"""K samples per pixel of a still view: the K-call loop (nrs_render_nerf + nrs_accumulate per sample) against one batch (nrs_render_nerf_spp + nrs_accumulate_spp).

For K in {1, 2, 4, 8, 16}, on bench.py's lego scene with its cage edit at 1920x1080 and on the scene without an edit at 256x256 (BASELINE configs[1]): both ways
are timed in one process, interleaved (loop, batch, loop, batch ...), HIP events around the whole K samples as bench.py times a frame; the frame slabs are cleared
outside the timed region for both.  Prints, per size and K, the median and the 10th..90th percentile spread of the ms per sample and the Gsamples/s of both, and
their ratio; --json adds one machine-readable line.

    python tools/spp_batch_probe.py [--reps 20] [--warmup 3] [--ks 1,2,4,8,16] [--json]
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ks", default="1,2,4,8,16")
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    import torch
    import bench
    from nerfshop_amd import runtime as rt, synth
    from nerfshop_amd._abi import check

    ctx = rt.Context(0)
    lib = ctx.lib
    rows = []
    for workload, (W, H) in (("lego_cage", (1920, 1080)), ("lego", (256, 256))):
        scene = bench.build_scene(workload, rt, synth, ctx, torch)
        tb = scene["tb"]
        n = W * H
        for K in [int(k) for k in args.ks.split(",")]:
            p = synth.render_params(W, H, bench.camera_for(2, synth, scene["aabb_scale"]), aabb_scale=scene["aabb_scale"], apply_operators=bool(tb.edit_operators),
                                    spp_index=0, snap=False)
            frames = torch.zeros((K, H, W, 4), dtype=torch.float32, device="cuda:0")
            depths = torch.zeros((K, H, W), dtype=torch.float32, device="cuda:0")
            accum = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")

            def loop(want_stats=False):
                samples = 0
                for k in range(K):
                    p.spp_index = k
                    st = tb.render_with_params(tb.nerf_network, p, frames[k], depths[k], None, None, want_stats)
                    check(lib.nrs_accumulate(ctx.h, None, W, H, frames[k].data_ptr(), accum.data_ptr(), k, 0))
                    samples += st.n_samples if want_stats else 0
                return samples

            def batch(want_stats=False):
                p.spp_index = 0
                st = tb.render_spp_with_params(tb.nerf_network, p, K, frames, depths, None, n, None, want_stats)
                check(lib.nrs_accumulate_spp(ctx.h, None, W, H, frames.data_ptr(), n, K, accum.data_ptr(), 0, 0))
                return st.n_samples if want_stats else 0

            frames.zero_()
            n_loop = loop(True)
            mean_loop = accum.clone()
            frames.zero_()
            n_batch = batch(True)
            torch.cuda.synchronize()
            assert n_loop == n_batch and torch.equal(mean_loop, accum), "the batch does not compute what the loop computes"
            ms = {"loop": [], "batch": []}
            for rep in range(args.warmup + args.reps):
                for name, fn in (("loop", loop), ("batch", batch)):
                    frames.zero_()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    torch.cuda.synchronize()
                    if rep >= args.warmup:
                        ms[name].append(e0.elapsed_time(e1) / K)
            row = {"workload": workload, "width": W, "height": H, "K": K, "samples_per_frame": n_loop // K}
            for name in ("loop", "batch"):
                v = np.asarray(ms[name])
                row[name] = {"ms_per_sample": round(float(np.median(v)), 4), "p10": round(float(np.quantile(v, 0.1)), 4), "p90": round(float(np.quantile(v, 0.9)), 4),
                             "gsamples_per_s": round(n_loop / K / float(np.median(v)) / 1e6, 3)}
            row["loop_over_batch"] = round(row["loop"]["ms_per_sample"] / row["batch"]["ms_per_sample"], 3)
            rows.append(row)
            print(f"{workload:9s} {W}x{H} K={K:2d}: loop {row['loop']['ms_per_sample']:.4f} ms/sample [{row['loop']['p10']:.4f} .. {row['loop']['p90']:.4f}] "
                  f"{row['loop']['gsamples_per_s']:.2f} Gsamples/s | batch {row['batch']['ms_per_sample']:.4f} ms/sample [{row['batch']['p10']:.4f} .. {row['batch']['p90']:.4f}] "
                  f"{row['batch']['gsamples_per_s']:.2f} Gsamples/s | loop / batch {row['loop_over_batch']:.3f}", flush=True)
        del scene, tb
    if args.json:
        print(json.dumps({"spp_batch_probe": rows, "device": ctx.device_name}))


if __name__ == "__main__":
    main()
