"""The display step at 1920x1080: nrs_tonemap (both output formats; the cheapest configuration, Identity linear -> linear, and the dearest, Hable sRGB -> sRGB),
nrs_accumulate in the same run as the yardstick of a kernel with known, similar traffic, and nrs_accumulate_spp + nrs_tonemap against nrs_accumulate_spp_tonemap for K = 8.

Every row is timed with HIP events on the stream around `--launches` back-to-back calls (one call is tens of microseconds: a single one would measure the event pair),
after `--warmup` untimed rounds, `--reps` times; the rows are interleaved round by round so that drift hits all of them alike.  Successive calls rotate through
`--sets` sets of buffers, so that a call does not find its input in the 256 MB last-level cache because the previous call left it there; --sets 1 shows the cached case.
Prints per row the median and the 10th..90th percentile of the microseconds per call, the bytes a call must move, their floor at 8 TB/s and floor / median; then the
ratios.  --json adds one machine-readable line.  Needs a GPU: there is nothing to fall back to.

    python tools/tonemap_probe.py [--reps 20] [--warmup 3] [--launches 48] [--sets 12] [--json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, K = 1920, 1080, 8
HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=48)
    ap.add_argument("--sets", type=int, default=12)
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    import torch
    from nerfshop_amd import _abi, runtime as rt
    from nerfshop_amd._abi import check

    ctx = rt.Context(0)
    lib = ctx.lib
    n = W * H
    g = torch.Generator().manual_seed(1)
    S = args.sets
    accs = [(torch.rand((n, 4), generator=g, dtype=torch.float32) * 1.5).to("cuda:0") for _ in range(S)]
    frames = [(torch.rand((n, 4), generator=g, dtype=torch.float32) * 1.5).to("cuda:0") for _ in range(S)]
    outs = [torch.empty((n, 4), dtype=torch.float32, device="cuda:0") for _ in range(S)]
    n_slab_sets = max(1, min(S, 3))   # 8 slabs are 265 MB: three sets already push one another out of the cache
    slabs = [(torch.rand((K, n, 4), generator=g, dtype=torch.float32) * 1.5).to("cuda:0") for _ in range(n_slab_sets)]

    def params(curve, space, fmt):
        t = _abi.TonemapParams()
        t.exposure = 1.0
        t.background_color[:] = (0.2, 0.5, 0.8, 0.6)
        t.color_space = t.output_color_space = space
        t.tonemap_curve, t.output_format = curve, fmt
        return t

    def tonemap_row(curve, space, fmt):
        t = params(curve, space, fmt)
        return lambda i: check(lib.nrs_tonemap(ctx.h, None, W, H, accs[i % S].data_ptr(), C.byref(t), outs[i % S].data_ptr()))

    def accumulate_row():
        # sample_count 5: the buffer is read (sample_count 0 overwrites it); Linear, so the values stay bounded however often the row runs
        return lambda i: check(lib.nrs_accumulate(ctx.h, None, W, H, frames[i % S].data_ptr(), accs[i % S].data_ptr(), 5, 0))

    def pair_row(fmt):
        t = params(_abi.TONEMAP_HABLE, 0, fmt)

        def call(i):
            check(lib.nrs_accumulate_spp(ctx.h, None, W, H, slabs[i % n_slab_sets].data_ptr(), n, K, accs[i % S].data_ptr(), 5, 0))
            check(lib.nrs_tonemap(ctx.h, None, W, H, accs[i % S].data_ptr(), C.byref(t), outs[i % S].data_ptr()))
        return call

    def fused_row(fmt):
        t = params(_abi.TONEMAP_HABLE, 0, fmt)
        return lambda i: check(lib.nrs_accumulate_spp_tonemap(ctx.h, None, W, H, slabs[i % n_slab_sets].data_ptr(), n, K, accs[i % S].data_ptr(), 5, C.byref(t), outs[i % S].data_ptr()))

    F32, U8 = _abi.TONEMAP_RGBA32F, _abi.TONEMAP_RGBA8
    # name -> (call, bytes per pixel a call must move)
    rows = {
        "tonemap rgba32f identity linear->linear": (tonemap_row(_abi.TONEMAP_IDENTITY, 0, F32), 16 + 16),
        "tonemap rgba32f hable srgb->srgb": (tonemap_row(_abi.TONEMAP_HABLE, 1, F32), 16 + 16),
        "tonemap rgba8 identity linear->linear": (tonemap_row(_abi.TONEMAP_IDENTITY, 0, U8), 16 + 4),
        "tonemap rgba8 hable srgb->srgb": (tonemap_row(_abi.TONEMAP_HABLE, 1, U8), 16 + 4),
        "accumulate linear": (accumulate_row(), 16 + 16 + 16),
        "accumulate_spp K=8 + tonemap rgba32f": (pair_row(F32), (K * 16 + 16 + 16) + (16 + 16)),
        "accumulate_spp_tonemap K=8 rgba32f": (fused_row(F32), K * 16 + 16 + 16 + 16),
        "accumulate_spp K=8 + tonemap rgba8": (pair_row(U8), (K * 16 + 16 + 16) + (16 + 4)),
        "accumulate_spp_tonemap K=8 rgba8": (fused_row(U8), K * 16 + 16 + 16 + 4),
    }
    us = {name: [] for name in rows}
    for rep in range(args.warmup + args.reps):
        for name, (call, _) in rows.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(args.launches):
                call(i)
            e1.record()
            torch.cuda.synchronize()
            if rep >= args.warmup:
                us[name].append(e0.elapsed_time(e1) * 1e3 / args.launches)
    table = {}
    for name, (_, bpp) in rows.items():
        v = np.asarray(us[name])
        floor = bpp * n / HBM_BYTES_PER_S * 1e6
        table[name] = {"us": round(float(np.median(v)), 2), "p10": round(float(np.quantile(v, 0.1)), 2), "p90": round(float(np.quantile(v, 0.9)), 2),
                       "mbytes": round(bpp * n / 1e6, 1), "floor_us": round(floor, 2), "floor_over_us": round(floor / float(np.median(v)), 3)}
        r = table[name]
        print(f"{name:42s} {r['us']:8.2f} us [{r['p10']:.2f} .. {r['p90']:.2f}]  {r['mbytes']:6.1f} MB  floor {r['floor_us']:6.2f} us  floor / measured {r['floor_over_us']:.3f}", flush=True)
    ratios = {
        "tonemap rgba32f dearest / cheapest": table["tonemap rgba32f hable srgb->srgb"]["us"] / table["tonemap rgba32f identity linear->linear"]["us"],
        "tonemap rgba8 dearest / cheapest": table["tonemap rgba8 hable srgb->srgb"]["us"] / table["tonemap rgba8 identity linear->linear"]["us"],
        "tonemap rgba8 / rgba32f (identity)": table["tonemap rgba8 identity linear->linear"]["us"] / table["tonemap rgba32f identity linear->linear"]["us"],
        "tonemap rgba32f (identity) / accumulate": table["tonemap rgba32f identity linear->linear"]["us"] / table["accumulate linear"]["us"],
        "pair / fused, rgba32f": table["accumulate_spp K=8 + tonemap rgba32f"]["us"] / table["accumulate_spp_tonemap K=8 rgba32f"]["us"],
        "pair / fused, rgba8": table["accumulate_spp K=8 + tonemap rgba8"]["us"] / table["accumulate_spp_tonemap K=8 rgba8"]["us"],
    }
    for name, v in ratios.items():
        print(f"{name:42s} {v:.3f}")
    if args.json:
        print(json.dumps({"tonemap_probe": table, "ratios": {k: round(v, 3) for k, v in ratios.items()}, "width": W, "height": H, "K": K, "launches": args.launches,
                          "sets": S, "reps": args.reps, "device": ctx.device_name}))


if __name__ == "__main__":
    main()
