"""The training-ray path at 2^20 samples: nrs_training_samples, nrs_network_inference, nrs_ray_loss and nrs_network_backward on the same batch: a first
measurement, no bar.  The batch is synthetic: rays whose sample counts are drawn (with replacement) from what the generator gives for rays shot at the bench scene
(synth.density_grid(1)) from outside its box, as many as fill 2^--log2-n samples, with random network outputs (densities spread so that about half the rays stop early).
nrs_training_samples is timed on the rays themselves (as many rays as the synthetic batch has).

The yardstick is nrs_network_inference at the same n; --parent-lib PATH names the libnrs.so built from a checkout of the parent commit (it must lack nrs_ray_loss),
loaded beside this tree's library (motion_blur_probe.package_with_library) and timed alternately with it.  Without it the yardstick row is this tree's.

Each call is timed with a pair of stream events (after `--warmup` untimed calls, `--reps` times: median and 10th..90th percentile).  Beside nrs_ray_loss's time: the
bytes it moves, computed from the shapes (per consumed sample the 8-byte outputs and the 4-byte dt in the forward pass, then outputs, the 28-byte record in and out
and 8 bytes of dL/doutput in the gradient pass; per ray its bookkeeping), over the time, against the 8 TB/s peak.
--json adds one machine-readable line.  Needs a GPU: there is nothing to fall back to.

    python tools/ray_loss_probe.py [--reps 7] [--warmup 2] [--log2-n 20] [--log2-hashmap 19] [--parent-lib PATH] [--json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8e12


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
    from nerfshop_amd import _abi, runtime as rt, synth
    from nerfshop_amd.torch_module import initial_params

    n = 1 << args.log2_n
    dev = "cuda:0"
    ctx = rt.Context(0)
    desc = synth.model_desc(1, log2_hashmap_size=args.log2_hashmap)
    net = rt.NerfNetwork(ctx, desc, cell_cache_bytes=0)
    n_params = net.n_params()
    params = initial_params(n_params, 7)
    params[10240:] *= 5e3
    net.set_params_device(params.to(torch.float16).cuda())
    net.set_density_bitfield(synth.grid_to_bitfield(synth.density_grid(1)))

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

    # rays at the scene from a sphere round it; their counts are the distribution the synthetic batch draws from
    rng = np.random.default_rng(11)
    n_probe = 1 << 14
    o = rng.normal(size=(n_probe, 3))
    o = 0.5 + 1.6 * o / np.linalg.norm(o, axis=1, keepdims=True)
    d = rng.uniform(0.25, 0.75, (n_probe, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    probe_rays = torch.from_numpy(np.concatenate([o, d], 1).astype(np.float32)).to(dev)
    _, numsteps, _, counters = net.training_samples(None, probe_rays, None, 0.0, n_probe * 256)
    hit = numsteps[:int(counters[0]), 0].cpu().numpy().astype(np.int64)
    counts = rng.choice(hit, size=2 * n // max(int(hit.mean()), 1) + 16)
    counts = counts[:int(np.searchsorted(np.cumsum(counts), n, side="right"))]
    R, used = len(counts), int(counts.sum())
    base = np.cumsum(counts) - counts
    numsteps = torch.from_numpy(np.stack([counts, base], 1).astype(np.int32)).to(dev)
    gen = torch.Generator(device=dev).manual_seed(3)
    coords = torch.rand((n, 7), generator=gen, device=dev) * 0.96 + 0.02
    coords[:, 3] = torch.rand(n, generator=gen, device=dev) * 0.2
    out = torch.empty((n, 16), dtype=torch.float16, device=dev)
    synthetic = (torch.randn((n, 16), generator=gen, device=dev) * 1.5).to(torch.float16)
    ray_of = torch.repeat_interleave(torch.arange(R, device=dev), torch.from_numpy(counts).to(dev))
    level = torch.randn(R, generator=gen, device=dev) * 1.5 + 3.0
    synthetic[:used, 3] = (level[ray_of] + torch.randn(used, generator=gen, device=dev)).clamp(-9, 9).to(torch.float16)
    target = torch.rand((R, 4), generator=gen, device=dev)
    target[:, 3] = 1.0
    p = _abi.RayLossParams(max_samples_compacted=n)
    bufs = (torch.empty_like(numsteps), torch.empty((n, 7), device=dev), torch.zeros((n, 16), dtype=torch.float16, device=dev), torch.empty(R, device=dev),
            torch.empty(1, dtype=torch.int32, device=dev))
    grad = torch.empty(n_params, dtype=torch.float32, device=dev)
    rays_all = probe_rays[torch.from_numpy(rng.integers(0, n_probe, R)).to(dev)].contiguous()

    rows = []
    g_coords, g_numsteps = torch.empty((n, 7), device=dev), torch.empty((R, 2), dtype=torch.int32, device=dev)
    g_idx, g_counters = torch.empty(R, dtype=torch.int32, device=dev), torch.empty(2, dtype=torch.int32, device=dev)
    stream = rt._stream_handle(None)

    def generate():  # the C call on buffers allocated once
        _abi.check(net.lib.nrs_training_samples(net.h, stream, R, rays_all.data_ptr(), None, 0.0, n, g_coords.data_ptr(), 7, g_numsteps.data_ptr(), g_idx.data_ptr(),
                                                g_counters.data_ptr()))

    med, lo, hi = timed(generate)
    rows.append({"step": f"nrs_training_samples ({R} rays, max_samples 2^{args.log2_n})", "ms": med, "p10": lo, "p90": hi})
    med, lo, hi = timed(lambda: net.inference_mixed_precision(None, coords, out))
    rows.append({"step": "nrs_network_inference, this tree", "ms": med, "p10": lo, "p90": hi})
    if args.parent_lib:
        from motion_blur_probe import package_with_library
        rt_p, synth_p = package_with_library("nerfshop_amd_parent", args.parent_lib)
        ctx_p = rt_p.Context(0)
        assert not hasattr(ctx_p.lib, "nrs_ray_loss"), "--parent-lib is not a library of the parent commit: it has the ray-loss entry point"
        net_p = rt_p.NerfNetwork(ctx_p, synth_p.model_desc(1, log2_hashmap_size=args.log2_hashmap), cell_cache_bytes=0)
        net_p.set_params_device(params.to(torch.float16).cuda())
        out_p = torch.empty_like(out)
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
        assert torch.equal(out_p.view(torch.int16), out.view(torch.int16)), "the parent's inference does not write what this tree's writes"
        for side in ("parent", "commit"):
            v = ts[side]
            rows.append({"step": f"nrs_network_inference, {side}, alternating", "ms": float(np.median(v)), "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90))})
    med, lo, hi = timed(lambda: net.ray_loss(None, p, numsteps, coords, synthetic, target, out=bufs))
    torch.cuda.synchronize()
    numsteps_out, consumed = bufs[0].cpu().numpy(), int(bufs[4][0])
    stopped = int((numsteps_out[:, 0] < counts).sum())
    moved = consumed * (12 + 8 + 28 + 28 + 8) + R * (8 + 16 + 36 + 8 + 36 + 8 + 4)
    rows.append({"step": f"nrs_ray_loss ({R} rays, {used} samples, {consumed} consumed, {stopped} rays stop early)", "ms": med, "p10": lo, "p90": hi, "bytes": moved,
                 "tb_per_s": moved / (med * 1e-3) / 1e12})
    med, lo, hi = timed(lambda: net.backward(None, bufs[1], bufs[2], grad, None, accumulate=False))
    rows.append({"step": "nrs_network_backward (n = max_samples_compacted, the compacted batch with its zero tail)", "ms": med, "p10": lo, "p90": hi})
    print(f"device: {ctx.device_name}   n = 2^{args.log2_n}   log2_hashmap_size {args.log2_hashmap}   mean samples per ray {counts.mean():.1f}")
    for row in rows:
        extra = f"  {row['bytes'] / 1e6:.1f} MB -> {row['tb_per_s']:.3f} TB/s ({row['tb_per_s'] * 1e12 / HBM_BYTES_PER_S * 100:.1f} % of 8 TB/s)" if "bytes" in row else ""
        print(f"{row['step']:100s} {row['ms']:9.3f} ms  [{row['p10']:.3f} .. {row['p90']:.3f}]{extra}")
    if args.json:
        print(json.dumps({"device": ctx.device_name, "n": n, "rays": R, "rows": rows}))


if __name__ == "__main__":
    main()
