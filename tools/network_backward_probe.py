"""nrs_network_backward at n = 2^20 random samples, log2_hashmap_size 19: a first measurement, no bar.  The yardstick is the PARENT COMMIT's nrs_network_inference
at the same n in the same run: --parent-lib PATH names the libnrs.so built from a checkout of the parent (it must lack nrs_network_backward); it is loaded into
this process beside this tree's library (motion_blur_probe.package_with_library), both run the same batch, their outputs must be equal bit for bit, and their
calls are timed alternately.  Without --parent-lib the yardstick row is this tree's nrs_network_inference and is labelled so.

Each call is timed with a pair of stream events (after `--warmup` untimed calls, `--reps` times: median and 10th..90th percentile).  Beside the time: the float
atomics a call issues -- 256 per sample into the grid gradient (16 levels x 8 corners x 2 features = 1 KB per sample) and 10 240 per workgroup for the MLP -- and
their floor at the chip-wide atomic rate of 1.3 TB/s.  Rows: random positions (every add of an instruction in another row of the table), the same batch sorted by
its finest level's cell (neighbouring lanes share entries), and random positions with overwrite (the memset) and with dL/dinput.
The counters behind the numbers take a run of their own (rocprofv3 --pmc ... -- python tools/network_backward_probe.py --reps 1 --warmup 0).
--json adds one machine-readable line.  Needs a GPU: there is nothing to fall back to.

    python tools/network_backward_probe.py [--reps 7] [--warmup 2] [--log2-n 20] [--log2-hashmap 19] [--parent-lib PATH] [--json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ATOMIC_BYTES_PER_S = 1.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log2-n", type=int, default=20)
    ap.add_argument("--log2-hashmap", type=int, default=19)
    ap.add_argument("--parent-lib", default=None, help="libnrs.so of the parent commit: its nrs_network_inference is the yardstick")
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    import torch
    from nerfshop_amd import runtime as rt, synth
    from nerfshop_amd.torch_module import initial_params

    n = 1 << args.log2_n
    ctx = rt.Context(0)
    desc = synth.model_desc(1, log2_hashmap_size=args.log2_hashmap)
    net = rt.NerfNetwork(ctx, desc, cell_cache_bytes=0)
    n_params = net.n_params()
    params = initial_params(n_params, 7)
    params[10240:] *= 5e3  # grid entries U(-0.5, 0.5): features of the size a trained snapshot has
    net.set_params_device(params.to(torch.float16).cuda())
    gen = torch.Generator(device="cuda:0").manual_seed(3)
    coords = torch.rand((n, 7), generator=gen, device="cuda:0") * 0.96 + 0.02
    scale15 = float(np.exp2(15 * np.log2(desc.per_level_scale)) * desc.base_resolution - 1.0)
    cell = (coords[:, :3] * scale15 + 0.5).floor().to(torch.int64)
    order = torch.argsort((cell[:, 2] * 4096 + cell[:, 1]) * 4096 + cell[:, 0])
    batches = {"random": coords, "sorted by finest cell": coords[order].contiguous()}
    dl = torch.zeros((n, 16), dtype=torch.float16, device="cuda:0")
    dl[:, :4] = torch.randn((n, 4), generator=gen, device="cuda:0").to(torch.float16)
    grad = torch.empty(n_params, dtype=torch.float32, device="cuda:0")
    din = torch.empty_like(coords)
    out = torch.empty((n, 16), dtype=torch.float16, device="cuda:0")

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ts = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts)), float(np.percentile(ts, 10)), float(np.percentile(ts, 90))

    n_wg = min((n + 255) // 256, ctx.n_cus)
    atomic_bytes = n * 256 * 4 + n_wg * 10240 * 4
    rows = []
    med, lo, hi = timed(lambda: net.inference_mixed_precision(None, coords, out))
    rows.append({"step": "nrs_network_inference, this tree (random)", "ms": med, "p10": lo, "p90": hi})
    t_fwd = med
    if args.parent_lib:
        from motion_blur_probe import package_with_library
        rt_p, synth_p = package_with_library("nerfshop_amd_parent", args.parent_lib)  # (its own ctypes classes: a description of its own)
        ctx_p = rt_p.Context(0)
        assert not hasattr(ctx_p.lib, "nrs_network_backward"), "--parent-lib is not a library of the parent commit: it has the backward entry point"
        net_p = rt_p.NerfNetwork(ctx_p, synth_p.model_desc(1, log2_hashmap_size=args.log2_hashmap), cell_cache_bytes=0)
        net_p.set_params_device(params.to(torch.float16).cuda())
        out_p = torch.empty_like(out)
        net_p.inference_mixed_precision(None, coords, out_p)
        torch.cuda.synchronize()
        assert torch.equal(out_p.view(torch.int16), out.view(torch.int16)), "the parent's inference does not write what this tree's writes"
        ts = {"parent": [], "commit": []}
        for rep in range(args.warmup + 2 * args.reps):
            for side in (("parent", "commit") if rep % 2 == 0 else ("commit", "parent")):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                (net_p if side == "parent" else net).inference_mixed_precision(None, coords, out_p if side == "parent" else out)
                e1.record()
                torch.cuda.synchronize()
                if rep >= args.warmup:
                    ts[side].append(e0.elapsed_time(e1))
        for side in ("parent", "commit"):
            v = ts[side]
            rows.append({"step": f"nrs_network_inference, {side}, alternating (random)", "ms": float(np.median(v)), "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90))})
        t_fwd = float(np.median(ts["parent"]))
    for name, c in batches.items():
        med, lo, hi = timed(lambda: net.backward(None, c, dl, grad, None, accumulate=True))
        rows.append({"step": f"nrs_network_backward ({name})", "ms": med, "p10": lo, "p90": hi, "x_inference": med / t_fwd, "atomic_bytes": atomic_bytes,
                     "floor_ms": atomic_bytes / ATOMIC_BYTES_PER_S * 1e3})
    med, lo, hi = timed(lambda: net.backward(None, coords, dl, grad, None, accumulate=False))
    rows.append({"step": "nrs_network_backward (random, overwrite: + memset)", "ms": med, "p10": lo, "p90": hi, "x_inference": med / t_fwd})
    med, lo, hi = timed(lambda: net.backward(None, coords, dl, grad, din, accumulate=True))
    rows.append({"step": "nrs_network_backward (random, + dL/dinput)", "ms": med, "p10": lo, "p90": hi, "x_inference": med / t_fwd})
    print(f"device: {ctx.device_name}   n = 2^{args.log2_n}   log2_hashmap_size {args.log2_hashmap}   {n_params} parameters")
    for row in rows:
        extra = f"  {row['x_inference']:6.2f} x inference" if "x_inference" in row else ""
        if "atomic_bytes" in row:
            extra += f"  atomics {row['atomic_bytes'] / 1e6:.0f} MB, floor {row['floor_ms']:.3f} ms ({row['floor_ms'] / row['ms']:.2f} of the time)"
        print(f"{row['step']:52s} {row['ms']:9.3f} ms  [{row['p10']:.3f} .. {row['p90']:.3f}]{extra}")
    if args.json:
        print(json.dumps({"device": ctx.device_name, "n": n, "log2_hashmap_size": args.log2_hashmap, "rows": rows}))


if __name__ == "__main__":
    main()
