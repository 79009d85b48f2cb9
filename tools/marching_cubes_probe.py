"""Mesh extraction at 256^3 and 512^3: a first measurement, no bar.  Two fields: a synthetic sphere (nrs_mesh_from_density alone) and the bench scene's density
(nrs_density_on_grid, nrs_mesh_from_density on its output, and nrs_mesh_extract = lattice + mesh + vertex colours).

nrs_mesh_from_density synchronises the stream, so a call is timed on the host's clock around it (after `--warmup` untimed calls, `--reps` times, median and 10th..90th
percentile); nrs_density_on_grid is asynchronous and is timed with a stream synchronisation either side.  The passes inside nrs_mesh_from_density (count, scan, emit,
1-ring) are not separated here: that takes a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/marching_cubes_probe.py --reps 1), whose per-kernel rows
carry the names mc_count_kernel, tile_scan_kernel<2>, mc_emit_kernel, mc_1ring_kernel, mesh_color_inputs_kernel, mesh_colors_kernel.  Beside every time: the bytes the
step must move (lattice read once per pass that reads it, per-point codes written once and read once, the mesh written once) and their floor at 8 TB/s.
--json adds one machine-readable line.  Needs a GPU: there is nothing to fall back to.

    python tools/marching_cubes_probe.py [--reps 7] [--warmup 2] [--sizes 256,512] [--json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    import torch
    from nerfshop_amd import runtime as rt, synth

    ctx = rt.Context(0)
    desc = synth.model_desc(1)
    tb = rt.Testbed(ctx, desc, 1)
    tb.nerf_network.set_params(synth.make_params(desc, sigma_raw=synth.default_sigma_raw(1), shaped=True))
    tb.nerf_network.set_density_grid(synth.density_grid(1))
    box = (list(desc.aabb_min), list(desc.aabb_max))

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), float(np.percentile(ts, 10)), float(np.percentile(ts, 90))

    rows = []
    print(f"device: {ctx.device_name}")
    for r in [int(v) for v in args.sizes.split(",")]:
        n = r ** 3
        ax = torch.arange(r, dtype=torch.float32, device="cuda:0") / r - 0.47
        sphere = (0.31 - torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)).contiguous()
        scene = tb.get_density_on_grid((r, r, r), box[0], box[1], mask_with_density_grid=False)
        thresh = float((scene.min() + scene.max()) / 2)
        for name, field, th in (("sphere", sphere, 0.0), ("scene", scene, thresh)):
            mesh = rt.mesh_from_density(ctx, field, box[0], box[1], th)
            nv, nt = mesh.n_verts_padded, mesh.n_tris
            # count reads the lattice and writes a code per point; emit reads both and writes the mesh; 1-ring reads the mesh's neighbourhoods and writes 28 B per vertex
            must = n * 4 + n * 4 + n * 4 + n * 4 + nv * (12 + 4) + nt * 12 + nv * (4 + 28) + nt * 12
            med, lo, hi = timed(lambda: rt.mesh_from_density(ctx, field, box[0], box[1], th))
            rows.append({"res": r, "field": name, "step": "nrs_mesh_from_density", "ms": med, "p10": lo, "p90": hi, "n_verts": mesh.n_verts, "n_tris": nt, "bytes": must,
                         "floor_ms": must / HBM_BYTES_PER_S * 1e3})
        med, lo, hi = timed(lambda: tb.get_density_on_grid((r, r, r), box[0], box[1], mask_with_density_grid=False))
        rows.append({"res": r, "field": "scene", "step": "nrs_density_on_grid", "ms": med, "p10": lo, "p90": hi, "bytes": n * (512 + 4), "floor_ms": n * 516 / HBM_BYTES_PER_S * 1e3})
        med, lo, hi = timed(lambda: tb.marching_cubes((r, r, r), box, thresh, mask_with_density_grid=False))
        rows.append({"res": r, "field": "scene", "step": "nrs_mesh_extract", "ms": med, "p10": lo, "p90": hi, "n_verts": tb.mesh.n_verts, "n_tris": tb.mesh.n_tris})
    for row in rows:
        extra = f"  must move {row['bytes'] / 1e6:9.1f} MB, floor {row['floor_ms']:.3f} ms ({row['floor_ms'] / row['ms']:.2f} of the time)" if "bytes" in row else ""
        mesh = f"  {row['n_verts']} vertices, {row['n_tris']} triangles" if "n_verts" in row else ""
        print(f"{row['res']:4d}^3 {row['field']:6s} {row['step']:22s} {row['ms']:8.3f} ms  [{row['p10']:.3f} .. {row['p90']:.3f}]{extra}{mesh}")
    if args.json:
        print(json.dumps({"device": ctx.device_name, "rows": rows}))


if __name__ == "__main__":
    main()
