"""Device buffers that are replaced or released while their owner lives on (nrs_host.h: DeviceBuffer), at the sites no other test drives:
the MVC weights of a cage operator set a second time with another cage, the dense and sparse cell records dropped and set again, and whole
create -> render -> destroy cycles of context, model and operator in one process.  The bar is the one the neighbouring tests hold: tables bit-equal to
the oracle's build (test_gpu_cage_update._check_tables), frames bit-equal to the frame without records (test_gpu_cell_cache) / to the first cycle's.
The smallest synthetic cage (lattice_n = 3), 64 x 36 frames, the documented destroy order (operators, model, context)."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 64, 36


def _same_bits(got, ref):
    return (np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)) and np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32))
            and np.array_equal(got[2], ref[2]) and got[3].n_samples == ref[3].n_samples)


def test_mvc_weights_replaced_by_another_cage(rig):
    """nrs_edit_set_mvc a second time with a different cage-vertex count (and back): the next nrs_edit_update_cage builds the oracle's tables."""
    from nerfshop_amd._abi import NrsError
    from test_gpu_cage_update import _check_tables
    scene = rig.scene
    synth, orc = scene.synth, scene.orc
    e = synth.make_cage_edit(lattice_n=3)
    small = types.SimpleNamespace(orc=orc, edit=e)
    n_v, n_cv = e.mvc_weights.shape
    # a cage of two more vertices: the old weights scaled, the rest on the new vertices, the same for every mesh vertex (the mesh shrinks and shifts, no tet
    # turns over; any weights do: the oracle applies the same matrix)
    wider = np.concatenate([np.float32(0.9) * e.mvc_weights, np.tile(np.float32([0.06, 0.04]), (n_v, 1))], axis=1).astype(np.float32)
    op = rig.rt.CageDeformation(rig.ctx, scene.desc, e, device_authoring=True)
    try:
        for weights, move in ((e.mvc_weights, ((0.02, 0.0, 0.01), 5.0)), (wider, ((0.05, -0.03, 0.02), 30.0)), (e.mvc_weights, ((0.10, 0.05, 0.0), 20.0))):
            op.set_mvc(weights)
            cage = synth.deform_cage(e.cage_vertices, *move)
            if weights.shape[1] != n_cv:
                with pytest.raises(NrsError):
                    op.update_cage(None, cage)   # the first cage's vertex count no longer fits
                cage = np.concatenate([cage, np.array([[0.55, 0.5, 0.45], [0.45, 0.55, 0.5]], np.float32)]).astype(np.float32)
            verts = orc.mvc_apply(weights, cage)
            op.update_cage(None, cage)
            _check_tables(op, small, verts)
    finally:
        op.close()


def test_cell_records_dropped_and_set_again(rig16):
    """nrs_model_set_cell_cache 0 -> two levels -> 0 -> two levels, then nrs_model_set_sparse_cell_cache set -> dropped (NULL mask) -> set again:
    the frame after every step is the frame without records, bit for bit."""
    from test_gpu_cell_cache import _level_cells
    rig, scene = rig16, rig16.scene
    two_levels = 32 * sum(_level_cells(scene.desc)[:2])
    mask = scene.bitfield
    rig.use_edit(False)
    try:
        rig.net.set_sparse_cell_cache(None, 0)
        rig.net.set_cell_cache(0)
        assert rig.net.cell_cache() == (0, 0) and rig.net.sparse_cell_cache() == (0, 0, 0)
        p = scene.params_for(W, H, 60.0)
        ref = rig.render(p)
        assert ref[3].n_samples > 1000
        for budget, want in ((two_levels, 2), (0, 0), (two_levels, 2)):
            rig.net.set_cell_cache(budget)
            assert rig.net.cell_cache() == (budget, want)
            assert _same_bits(rig.render(p), ref), budget
        sparse = []
        for m in (mask, None, mask):
            rig.net.set_sparse_cell_cache(m, (2 << 30) if m is not None else 0)
            sparse.append(rig.net.sparse_cell_cache())
            assert _same_bits(rig.render(p), ref), sparse
        assert sparse[0][1] == 2 and sparse[0][2] >= 2 and sparse[0][0] > 0, sparse   # records of the levels behind the two dense ones
        assert sparse[1] == (0, 0, 0) and sparse[2] == sparse[0], sparse
    finally:
        rig.net.set_sparse_cell_cache(None, 0)
        rig.net.set_cell_cache(10 << 30)


def test_create_render_destroy_cycles(scene):
    """Three lives of context, model and cage operator in one process: every cycle renders the first cycle's frame."""
    import torch
    from nerfshop_amd import runtime
    synth = scene.synth
    e = synth.make_cage_edit(lattice_n=3)
    cage = synth.deform_cage(e.cage_vertices, (0.05, -0.03, 0.02), 30.0)
    p = scene.params_for(W, H, 60.0)
    frames = []
    for _ in range(3):
        ctx = runtime.Context(0)
        tb = runtime.Testbed(ctx, scene.desc, 1)
        tb.nerf_network.set_params(scene.params)
        tb.nerf_network.set_density_bitfield(scene.bitfield)
        op = runtime.CageDeformation(ctx, scene.desc, e, device_authoring=True)
        op.set_mvc(e.mvc_weights)
        op.update_cage(None, cage)
        tb.add_edit_operator(op)
        frame = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
        depth = torch.zeros((H, W), dtype=torch.float32, device="cuda:0")
        steps = torch.zeros((H, W), dtype=torch.int32, device="cuda:0")
        stats = tb.render_with_params(tb.nerf_network, p, frame, depth, steps, None, want_stats=True)
        torch.cuda.synchronize()
        frames.append((frame.cpu().numpy(), depth.cpu().numpy(), steps.cpu().numpy(), stats))
        op.close()
        tb.nerf_network.close()
        ctx.close()
    assert frames[0][3].n_samples > 1000
    for k in (1, 2):
        assert _same_bits(frames[k], frames[0]), k
