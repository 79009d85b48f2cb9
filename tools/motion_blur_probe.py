"""K samples of a motion-blurred frame: the K-call loop with per-sample cameras (nrs_render_nerf + nrs_accumulate per sample) against one views batch
(nrs_render_nerf_spp_views + nrs_accumulate_spp), with the still batch of the same K (nrs_render_nerf_spp) timed beside them.

For K in {2, 8, 16}, on bench.py's lego scene with its cage edit at 1920x1080 and on the scene without an edit at 256x256; the camera turns about 1 degree over the
frame (nrs_motion_views between two cameras, shutter 1).  The three arms run in one process, interleaved, 3 warm-up + 20 timed repetitions, HIP events around the K
samples, the frame slabs cleared outside the timed region.  Prints the median and the 10th..90th percentile of the ms per sample of each arm; --json adds one line.

--parent-lib PATH adds the A/B of the still batch: the libnrs.so of the parent commit (built from a checkout of it) is loaded into the same process beside this
tree's, and nrs_render_nerf_spp + nrs_accumulate_spp of lego + cage at 1920x1080, K = 8, runs on both, interleaved, after a check that both write the same bits.
The verdict line says whether this tree's median lies inside the parent's own 10th..90th percentile range.

    python tools/motion_blur_probe.py [--reps 20] [--warmup 3] [--ks 2,8,16] [--parent-lib PATH] [--json]
"""
import importlib
import importlib.util
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def turned(cam, degrees):
    a = np.deg2rad(degrees)
    rot = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    m = np.asarray(list(cam), np.float64).reshape(4, 3).T
    out = np.empty((3, 4))
    out[:, :3] = rot @ m[:, :3]
    out[:, 3] = rot @ (m[:, 3] - 0.5) + 0.5
    return [float(v) for v in out.T.reshape(-1).astype(np.float32)]


def package_with_library(name, lib_path):
    """(runtime, synth) of a second copy of the nerfshop_amd package bound to another libnrs.so (_abi reads NRS_LIB_PATH when it is imported)"""
    pkg = os.path.join(ROOT, "nerfshop_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    old = os.environ.get("NRS_LIB_PATH")
    os.environ["NRS_LIB_PATH"] = os.path.abspath(lib_path)
    try:
        spec.loader.exec_module(mod)
        out = importlib.import_module(name + ".runtime"), importlib.import_module(name + ".synth")
        importlib.import_module(name + "._abi").load()
    finally:
        if old is None:
            del os.environ["NRS_LIB_PATH"]
        else:
            os.environ["NRS_LIB_PATH"] = old
    return out


def quantiles(v):
    v = np.asarray(v)
    return {"ms_per_sample": round(float(np.median(v)), 4), "p10": round(float(np.quantile(v, 0.1)), 4), "p90": round(float(np.quantile(v, 0.9)), 4)}


def still_batch_against_parent(args, torch, bench, rt, synth, ctx):
    """the still batch of lego + cage, 1920x1080, K = 8: this tree's library against the parent's, both in this process"""
    W, H, K = 1920, 1080, 8
    n = W * H
    rt_p, synth_p = package_with_library("nerfshop_amd_parent", args.parent_lib)
    # both libraries define the same C symbols: the A/B means something only if each side's handle is its own file (ctypes opens them RTLD_LOCAL)
    lib_p = sys.modules["nerfshop_amd_parent._abi"].load()
    assert os.path.realpath(lib_p._name) != os.path.realpath(ctx.lib._name), f"both sides are bound to {ctx.lib._name}"
    assert hasattr(ctx.lib, "nrs_render_nerf_spp_views") and not hasattr(lib_p, "nrs_render_nerf_spp_views"), "--parent-lib is not a library of the parent commit: it has the views entry point"
    sides = {}
    for side, (r, s, c) in (("parent", (rt_p, synth_p, rt_p.Context(0))), ("commit", (rt, synth, ctx))):
        scene = bench.build_scene("lego_cage", r, s, c, torch)
        p = s.render_params(W, H, bench.camera_for(2, s, scene["aabb_scale"]), aabb_scale=scene["aabb_scale"], apply_operators=True, spp_index=0, snap=False)
        sides[side] = (scene, p, c)
    frames = torch.zeros((K, H, W, 4), dtype=torch.float32, device="cuda:0")
    depths = torch.zeros((K, H, W), dtype=torch.float32, device="cuda:0")
    accum = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")

    def still(side):
        scene, p, c = sides[side]
        tb = scene["tb"]
        tb.render_spp_with_params(tb.nerf_network, p, K, frames, depths, None, n, None, False)
        check = sys.modules[type(tb).__module__]._abi.check
        check(c.lib.nrs_accumulate_spp(c.h, None, W, H, frames.data_ptr(), n, K, accum.data_ptr(), 0, 0))

    seen = {}
    for side in sides:
        frames.zero_(); depths.zero_()
        still(side)
        torch.cuda.synchronize()
        seen[side] = (frames.clone(), depths.clone(), accum.clone())
    assert all(torch.equal(a, b) for a, b in zip(seen["parent"], seen["commit"])), "the still batch of this tree does not write what the parent's writes"
    del seen
    ms = {side: [] for side in sides}
    for rep in range(args.warmup + args.reps):
        for side in (("parent", "commit") if rep % 2 == 0 else ("commit", "parent")):
            frames.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            still(side)
            e1.record()
            torch.cuda.synchronize()
            if rep >= args.warmup:
                ms[side].append(e0.elapsed_time(e1) / K)
    row = {"workload": "lego_cage", "width": W, "height": H, "K": K, "parent": quantiles(ms["parent"]), "commit": quantiles(ms["commit"])}
    row["commit_inside_parent_p10_p90"] = bool(row["parent"]["p10"] <= row["commit"]["ms_per_sample"] <= row["parent"]["p90"])
    row["commit_over_parent"] = round(row["commit"]["ms_per_sample"] / row["parent"]["ms_per_sample"], 4)
    print("still batch, lego_cage 1920x1080 K= 8: " + " | ".join(f"{side} {row[side]['ms_per_sample']:.4f} ms/sample [{row[side]['p10']:.4f} .. {row[side]['p90']:.4f}]" for side in sides) +
          f" | commit / parent {row['commit_over_parent']:.4f} | commit's median inside the parent's p10..p90: {row['commit_inside_parent_p10_p90']}", flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libnrs.so of the parent commit: adds the still batch A/B")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ks", default="2,8,16")
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    import torch
    import bench
    from nerfshop_amd import _abi, runtime as rt, synth
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
            base = _abi.SampleView()
            base.focal_length[:] = list(p.focal_length)
            base.dof, base.slice_plane_z = p.dof, p.slice_plane_z
            cam0 = list(p.camera_matrix0)
            views = tb.motion_views(cam0, turned(cam0, 1.0), 1.0, K, 0, K, (W, H), -1.0, -1.0, base)
            frames = torch.zeros((K, H, W, 4), dtype=torch.float32, device="cuda:0")
            depths = torch.zeros((K, H, W), dtype=torch.float32, device="cuda:0")
            accum = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
            q = _abi.RenderParams()

            def loop(want_stats=False):
                samples = 0
                for k in range(K):
                    _abi.C.pointer(q)[0] = p
                    q.spp_index = k
                    q.camera_matrix0[:] = list(views[k].camera_matrix0); q.camera_matrix1[:] = list(views[k].camera_matrix1)
                    st = tb.render_with_params(tb.nerf_network, q, frames[k], depths[k], None, None, want_stats)
                    check(lib.nrs_accumulate(ctx.h, None, W, H, frames[k].data_ptr(), accum.data_ptr(), k, 0))
                    samples += st.n_samples if want_stats else 0
                return samples

            def batch(want_stats=False):
                p.spp_index = 0
                st = tb.render_spp_with_views(tb.nerf_network, p, views, frames, depths, None, n, None, want_stats)
                check(lib.nrs_accumulate_spp(ctx.h, None, W, H, frames.data_ptr(), n, K, accum.data_ptr(), 0, 0))
                return st.n_samples if want_stats else 0

            def still(want_stats=False):
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
            assert n_loop == n_batch and torch.equal(mean_loop, accum), "the views batch does not compute what the loop computes"
            arms = (("loop", loop), ("views_batch", batch), ("still_batch", still))
            ms = {name: [] for name, _ in arms}
            for rep in range(args.warmup + args.reps):
                for name, fn in arms:
                    frames.zero_()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    torch.cuda.synchronize()
                    if rep >= args.warmup:
                        ms[name].append(e0.elapsed_time(e1) / K)
            row = {"workload": workload, "width": W, "height": H, "K": K, "samples_per_frame": n_loop // K}
            for name, _ in arms:
                row[name] = quantiles(ms[name])
            row["loop_over_views_batch"] = round(row["loop"]["ms_per_sample"] / row["views_batch"]["ms_per_sample"], 3)
            rows.append(row)
            print(f"{workload:9s} {W}x{H} K={K:2d}: " + " | ".join(f"{name} {row[name]['ms_per_sample']:.4f} ms/sample [{row[name]['p10']:.4f} .. {row[name]['p90']:.4f}]" for name, _ in arms) +
                  f" | loop / views batch {row['loop_over_views_batch']:.3f}", flush=True)
        del scene, tb
    ab = still_batch_against_parent(args, torch, bench, rt, synth, ctx) if args.parent_lib else None
    if args.json:
        print(json.dumps({"motion_blur_probe": rows, "still_batch_against_parent": ab, "device": ctx.device_name}))


if __name__ == "__main__":
    main()
