"""Child process of tests/test_gpu_light_dirs.py: renders of a model with light directions under development knobs, which are read from the environment of a
process (NRS_DEV_KNOBS=1 set by the parent for this process only).  No oracle.
usage: light_worker.py refuse   -- NRS_DEBUG=4 or NRS_RENDER_CFG=84 in the environment: prints "light <case> status <s> <message>" for a plain frame, an AO frame and
                                   a batch of a light model, and "plain status <s>" for a plain model
       light_worker.py routes   -- NRS_KERNEL_LOG=1: prints "[route <case>] <instantiation>" for every case, the instantiation as the kernel log names it"""
import ctypes as C
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    mode = sys.argv[1]
    import numpy as np
    import torch
    from nerfshop_amd import _abi, runtime as rt, synth
    W, H = 64, 48
    ctx = rt.Context(0)
    lib = ctx.lib
    desc = synth.model_desc(1)
    bitfield = synth.grid_to_bitfield(synth.density_grid(1))

    def light_testbed(d):
        tb = rt.Testbed(ctx, d, 1, n_extra_dims=3)
        tb.nerf_network.set_params(synth.make_light_params(d, sigma_raw=synth.default_sigma_raw(1)))
        tb.nerf_network.set_density_bitfield(bitfield)
        return tb
    tb = light_testbed(desc)
    frames = torch.zeros((2, H, W, 4), dtype=torch.float32, device="cuda:0")
    depths = torch.zeros((2, H, W), dtype=torch.float32, device="cuda:0")

    def params(**fields):
        p = synth.render_params(W, H, synth.orbit_camera(30.0), snap=False)
        for k, v in fields.items():
            setattr(p, k, v)
        return p

    def render(t, p, batch=False):
        """-> (status, message) of one call through the C-ABI"""
        n = len(t.edit_operators)
        arr = (C.c_void_p * max(n, 1))(*[op.h for op in t.edit_operators])
        if batch:
            st = lib.nrs_render_nerf_spp(t.nerf_network.h, C.byref(p), arr, n, 2, frames.data_ptr(), depths.data_ptr(), None, W * H, None, None)
        else:
            st = lib.nrs_render_nerf(t.nerf_network.h, C.byref(p), arr, n, frames[0].data_ptr(), depths[0].data_ptr(), None, None, None)
        torch.cuda.synchronize()
        return st, lib.nrs_last_error().decode() if st else ""

    if mode == "refuse":
        for case, p, batch in (("plain", params(), False), ("ao", params(render_mode=_abi.RENDER_AO), False), ("batch", params(), True)):
            st, msg = render(tb, p, batch)
            print(f"light {case} status {st} {msg}", flush=True)
        plain = rt.Testbed(ctx, desc, 1)
        plain.nerf_network.set_params(synth.make_params(desc, sigma_raw=synth.default_sigma_raw(1)))
        plain.nerf_network.set_density_bitfield(bitfield)
        print(f"plain status {render(plain, params())[0]}", flush=True)
        return

    # routes: the kernel log goes to the C library's stderr (file descriptor 2): point it at a file around each case
    def logged(case, t, p, batch=False):
        sys.stderr.flush()
        with tempfile.TemporaryFile(mode="w+") as f:
            saved = os.dup(2)
            os.dup2(f.fileno(), 2)
            try:
                st, msg = render(t, p, batch)
            finally:
                os.dup2(saved, 2)
                os.close(saved)
            f.seek(0)
            names = [l[len("[nrs kernel] "):].strip() for l in f.read().splitlines() if l.startswith("[nrs kernel] ")]
        assert st == 0, (case, st, msg)
        assert len(names) == 1, (case, names)
        print(f"[route {case}] {names[0]}", flush=True)

    logged("plain", tb, params())
    logged("batch", tb, params(), batch=True)
    edit = synth.make_cage_edit(lattice_n=4)
    tb.edit_operators = [rt.CageDeformation(ctx, desc, edit)]
    logged("cage", tb, params())
    tb.edit_operators = [rt.AffineDuplication(ctx, desc, synth.make_affine_edit())]
    logged("affine", tb, params())
    tb.edit_operators = []
    tb.nerf_network.set_numerics(1, 1)
    logged("numerics", tb, params())
    tb.nerf_network.set_numerics(0, 0)
    logged("ao", tb, params(render_mode=_abi.RENDER_AO))
    logged("ao_batch", tb, params(render_mode=_abi.RENDER_AO), batch=True)
    ctx.set_lane_teams(2)
    logged("teams", tb, params())
    ctx.set_lane_teams(0)
    logged("deep", light_testbed(synth.model_desc(1, rgb_hidden_layers=3)), params())


if __name__ == "__main__":
    main()
