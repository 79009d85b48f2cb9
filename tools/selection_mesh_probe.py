"""The selection tool's device side on the synthetic scene: scribble -> reset_growing -> grow_region (0.01, 10 000) -> the closing (dilation Cube 2, erosion Sphere 2)
and the fine mesh.  A first measurement, no bar.

  closing, device   two nrs_bitfield_morph calls (each: pack to rows, the morphology kernel, unpack, two memsets) on a device copy of the selection bitfield, timed with
                    events round `--reps` repetitions after `--warmup` untimed ones
  closing, host     the same two operations through nrs_bitfield_morph_host on one CPU thread, wall time (median of 3)
  lattice + mesh    nrs_selection_fine_mesh without morphology (the rows upload, the lattice kernel, nrs_mesh_from_density's code, its two synchronisations), wall time
  closing + mesh    nrs_selection_fine_mesh with morphology on a freshly grown selection, wall time (includes the copy back and the rebuild of the cell list on the host)

The figures go to stdout as a markdown section; --out appends them to a file (profiles/selection_mesh.md keeps the last run).  Needs a GPU: there is nothing to fall back to.

    python tools/selection_mesh_probe.py [--reps 20] [--warmup 3] [--commit <id>] [--out profiles/selection_mesh.md]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from nerfshop_amd import _abi, runtime as rt, synth

    commit = args.commit
    if commit is None:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 and r.stdout.strip() else "unknown (not a git checkout)"

    ctx = rt.Context(0)
    desc = synth.model_desc(1)
    tb = rt.Testbed(ctx, desc, 1)
    tb.nerf_network.set_params(synth.make_params(desc, sigma_raw=synth.default_sigma_raw(1)))
    grid = synth.density_grid(1)
    tb.nerf_network.set_density_grid(grid)
    w, h = 640, 360
    rng = np.random.default_rng(11)
    px = np.stack([rng.integers(w // 4, 3 * w // 4, 400), rng.integers(h // 4, 3 * h // 4, 400)], 1).astype(np.int32)
    p = synth.render_params(w, h, synth.orbit_camera(50.0, 30.0, scale=0.33))
    _, (cells, _, level) = tb.project_selection_pixels(p, px)

    def grown():
        sel = tb.growing_selection(max_cascade=0)
        sel.reset_growing(cells, level)
        sel.grow_region()
        return sel

    sel = grown()
    bits = sel.selection_grid_bitfield
    n_selected = int(np.unpackbits(bits).sum())
    d_in = torch.as_tensor(bits, device="cuda:0")
    d_mid, d_out = torch.empty_like(d_in), torch.empty_like(d_in)

    def closing():
        rt.bitfield_morph(ctx, d_in, level, _abi.MORPH_DILATE, _abi.SE_CUBE, 2, out=d_mid)
        rt.bitfield_morph(ctx, d_mid, level, _abi.MORPH_ERODE, _abi.SE_SPHERE, 2, out=d_out)

    for _ in range(args.warmup):
        closing()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        closing()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        closing()
    e1.record()
    e1.synchronize()
    back_to_back = e0.elapsed_time(e1) / args.reps
    device_result = d_out.cpu().numpy()

    host_times = []
    for _ in range(3):
        t0 = time.perf_counter()
        mid = rt.bitfield_morph_host(bits, level, _abi.MORPH_DILATE, _abi.SE_CUBE, 2)
        host_result = rt.bitfield_morph_host(mid, level, _abi.MORPH_ERODE, _abi.SE_SPHERE, 2)
        host_times.append((time.perf_counter() - t0) * 1e3)
    same = bool(np.array_equal(device_result, host_result))

    def wall(fn, reps):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), float(min(ts)), float(max(ts))

    sel.use_morphological = False
    sel.extract_fine_mesh()
    plain = wall(sel.extract_fine_mesh, args.reps)
    plain_tris = sel.selection_mesh.n_tris
    closed_times = []
    for _ in range(5):
        s2 = grown()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mesh = s2.extract_fine_mesh()
        closed_times.append((time.perf_counter() - t0) * 1e3)
        closed_tris, closed_cells = mesh.n_tris, len(s2.selection_cell_idx)
        s2.close()

    lines = [
        f"## Run on {ctx.device_name}, commit {commit}",
        "",
        f"Selection: {len(cells)} seed cells at level {level}, {n_selected} cells after `grow_region(0.01, 10000)`; {closed_cells} after the closing.",
        f"Device and host closings bit-equal: {same}.",
        "",
        "| what | time | how |",
        "|---|---|---|",
        f"| closing on the device, one at a time | median {np.median(times) * 1e3:.1f} us, min {min(times) * 1e3:.1f}, max {max(times) * 1e3:.1f} | events round each of {args.reps} repetitions (6 kernels, 4 memsets) after {args.warmup} warm-ups |",
        f"| closing on the device, back to back | {back_to_back * 1e3:.1f} us per closing | one pair of events round {args.reps} repetitions |",
        f"| closing on the host, one thread | median {np.median(host_times):.1f} ms, min {min(host_times):.1f} | wall time of two `nrs_bitfield_morph_host` calls, 3 repetitions |",
        f"| lattice + mesh (`nrs_selection_fine_mesh`, no morphology) | median {plain[0]:.3f} ms, min {plain[1]:.3f}, max {plain[2]:.3f} | wall time of the synchronous call, {args.reps} repetitions; {plain_tris} triangles |",
        f"| closing + lattice + mesh (`nrs_selection_fine_mesh`, morphology) | median {np.median(closed_times):.3f} ms, min {min(closed_times):.3f} | wall time of the synchronous call on a freshly grown selection, 5 repetitions; includes the copy back and the host's rebuild of the cell list; {closed_tris} triangles |",
        "",
    ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
