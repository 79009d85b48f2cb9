"""Child process of tests/test_gpu_occupancy_training.py test_cell_order_equals_sample_order: occupancy_ref.WORKER_CASES' refreshes on cuda:0, no oracle.  The parent
starts it with NRS_DEV_KNOBS=1 NRS_REFRESH_ORDER=0 (grid_refresh_kernel then walks the samples in their own order) and hands over the start grids as
<dir>/start_<case>.npy; the child writes grid, bitfield and (ema_step, rng_state, rng_inc) of each case to <dir>/out_<case>.npz.
usage: occupancy_worker.py <dir>"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import numpy as np
    import occupancy_ref as oref
    from nerfshop_amd import runtime, synth
    assert os.environ.get("NRS_DEV_KNOBS") == "1" and os.environ.get("NRS_REFRESH_ORDER") == "0", "the parent sets the sample-order knob"
    work = sys.argv[1]
    ctx = runtime.Context(0)
    for name in oref.WORKER_CASES:
        case = oref.CASES[name]
        aabb_scale = {"shaped": 1, "shaped16": 16}[case["scene"]]
        desc = synth.model_desc(aabb_scale)
        # conftest's Scene(shaped=True) parameters of this aabb_scale
        params = synth.make_params(desc, sigma_raw=synth.default_sigma_raw(aabb_scale), shaped=True, aabb_scale=aabb_scale)
        net = runtime.NerfNetwork(ctx, desc, cell_cache_bytes=0)
        net.set_params(params)
        net.set_density_grid(np.load(os.path.join(work, f"start_{name}.npy")))
        u = oref.grid_update(case)
        net.update_density_grid(u)
        np.savez(os.path.join(work, f"out_{name}.npz"), grid=net.get_density_grid(), bits=net.get_density_bitfield(),
                 state=np.array([u.ema_step, u.rng_state, u.rng_inc], np.uint64))
    print(f"refreshes in sample order: {len(oref.WORKER_CASES)}", flush=True)


if __name__ == "__main__":
    main()
