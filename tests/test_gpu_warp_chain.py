"""The cage operator's memory chain (nrs_edit_warp.cuh find_tet / scan_fine_cell_for_tet / tet_warp): the fine window through scalar loads, the head word per fine
cell (DeviceEdit::fine_head) and the map-back record per tet (DeviceEdit::mapback) change which loads bring the operands, not one float operation.  So
CageDeformation.map_rays / map_positions must give the oracle's operator (cage_deformation.cu:136-269 restated on the CPU) bit for bit: coordinates, directions and
the empty mask, in every state an operator goes through -- as created (fine table with heads), after a cage move (table dropped: the plain scan, map-back records
with the rotations of the new pose) and after the frame at rest that rebuilds the table.

The fallback without head words (an edit of 2^25 tets or more) is reached through the measurement knob NRS_NO_FINE_HEAD, in a process of its own."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1 << 16
FAR_BOX = ((2.35, 0.55, 0.35), (2.65, 0.80, 0.65))   # straddles |x - 0.5| = 2: cascades 2 and 3 of a scene box of scale 16


def _make_edit(synth, lattice, aabb_scale, rot=True, copy=False):
    """aabb_scale 1: the bench's cage.  aabb_scale 16: a cage of the same size far from the centre, across the border of cascades 2 and 3 -- neighbouring points
    (lanes of one wave) stand in different cascades, and with lattice 10 a cell of cascades 3 and 4 holds more than kFineMaxList tets (kFinePlain: the LUT's own lists)."""
    if aabb_scale == 1:
        return synth.make_cage_edit(lattice_n=lattice, copy=copy, correct_direction=rot)
    return synth.make_cage_edit(lattice_n=lattice, box=FAR_BOX, translate=(0.05, 0.03, -0.02), copy=copy, correct_direction=rot)


def _posed(synth, edit, cage_pose):
    """the host arrays of `edit` with its cage at cage_pose: what the oracle's operator is created from"""
    import copy as _copy
    e = _copy.copy(edit)
    e.vertices = np.ascontiguousarray(synth.mvc_apply(edit.mvc_weights, cage_pose), np.float32)
    off, idx, _, mx = synth.build_tet_lut(e.vertices, e.tets)
    e.lut_offsets, e.lut_idx, e.max_per_cell = off, (idx if idx.size else np.zeros(1, np.uint32)), mx
    e.local_rotations = synth.local_rotations(e.vertices, e.original_vertices, e.tets) if edit.local_rotations is not None else None
    return e


def _batch(synth, edit, verts, aabb_scale, seed):
    """N warped coordinates [N, 7], drawn like tests/test_gpu_fine_lut.py draws them: uniform in the deformed box plus a margin (at scale 16 an eighth over the whole
    scene box), a fifth ON vertices / edge midpoints / face centres of tets and a hair beside them -- where the list ORDER decides which tet is found"""
    rng = np.random.default_rng(seed)
    n = N
    mn, mx = (np.array(v, np.float32) for v in synth.scene_aabb(aabb_scale))
    lo, hi = verts.min(0), verts.max(0)
    ext = hi - lo
    world = rng.uniform(lo - 0.03 * ext, hi + 0.03 * ext, size=(n, 3)).astype(np.float32)
    if aabb_scale != 1:
        world[-n // 8:] = rng.uniform(mn, mx, size=(n // 8, 3)).astype(np.float32)
    t = edit.tets[rng.integers(0, edit.tets.shape[0], n // 5)]
    w = rng.dirichlet([0.4, 0.4, 0.4, 0.4], size=n // 5).astype(np.float32)
    eye = np.eye(4, dtype=np.float32)
    w[: n // 15] = eye[rng.integers(0, 4, n // 15)]
    w[n // 15: 2 * n // 15] = 0.5 * (eye[rng.integers(0, 4, n // 15)] + eye[rng.integers(0, 4, n // 15)])
    world[: n // 5] = np.einsum("nk,nkd->nd", w, verts[t]).astype(np.float32)
    world[n // 10: n // 5] += rng.normal(0, 2e-7, size=(n // 5 - n // 10, 3)).astype(np.float32) * np.float32(np.abs(verts).max())
    world = world[rng.permutation(n)]   # (the points on the tets are spread over the waves)
    c = np.zeros((n, 7), np.float32)
    c[:, :3] = (world - mn) / (mx - mn)
    c[:, 3] = 1e-3
    d = rng.normal(size=(n, 3))
    c[:, 4:] = ((d / np.linalg.norm(d, axis=1, keepdims=True) + 1.0) * 0.5).astype(np.float32)
    return c


def _gpu_maps(torch, op, c):
    dc = torch.from_numpy(c).cuda()
    mask = torch.zeros(c.shape[0], dtype=torch.uint8, device="cuda:0")
    op.map_rays(None, dc, mask)
    dp = torch.from_numpy(np.ascontiguousarray(c[:, :3])).cuda()
    mask2 = torch.zeros(c.shape[0], dtype=torch.uint8, device="cuda:0")
    op.map_positions(None, dp, mask2)
    torch.cuda.synchronize()
    return dc.cpu().numpy(), mask.cpu().numpy(), dp.cpu().numpy(), mask2.cpu().numpy()


def _rest_frames(rt, synth, ctx, desc, op, aabb_scale):
    """two small frames through the operator: the second one after a move builds the fine table of the new pose (nrs_edit::fine_stale)"""
    import torch
    tb = rt.Testbed(ctx, desc, aabb_scale)
    tb.nerf_network.set_cell_cache(0)
    tb.nerf_network.set_params(synth.make_params(desc, sigma_raw=synth.default_sigma_raw(aabb_scale)))
    tb.nerf_network.set_density_bitfield(synth.grid_to_bitfield(synth.density_grid(aabb_scale)))
    tb.add_edit_operator(op)
    p = synth.render_params(64, 36, synth.orbit_camera(30.0, 30.0, scale=0.33 if aabb_scale == 1 else 0.33 * 6.0), aabb_scale=aabb_scale)
    frame = torch.zeros((36, 64, 4), device="cuda:0")
    depth = torch.zeros((36, 64), device="cuda:0")
    for _ in range(2):
        tb.render_with_params(tb.nerf_network, p, frame, depth, None, None)
    torch.cuda.synchronize()


def _states(rt, synth, ctx, desc, edit, aabb_scale):
    """yields (state, deformed vertices of the state, the operator) for: created, moved, rested"""
    op = rt.CageDeformation(ctx, desc, edit, device_authoring=True)
    op.set_mvc(edit.mvc_weights)
    yield "created", edit.vertices, edit.cage_deformed, op
    ext = float(np.ptp(edit.cage_vertices, axis=0).max())
    pose = synth.deform_cage(edit.cage_vertices, (0.18 * ext, 0.08 * ext, -0.05 * ext), 33.0)
    op.update_cage(None, pose)
    verts2 = np.ascontiguousarray(synth.mvc_apply(edit.mvc_weights, pose), np.float32)
    yield "moved", verts2, pose, op
    _rest_frames(rt, synth, ctx, desc, op, aabb_scale)
    yield "rested", verts2, pose, op
    op.close()


@pytest.mark.parametrize("lattice,aabb_scale,rot,copy", [(2, 1, True, False), (10, 1, True, False), (2, 16, True, False), (10, 16, True, False),
                                                         (10, 1, False, False), (10, 1, True, True)])
def test_operator_is_the_oracles_in_every_state(built, lattice, aabb_scale, rot, copy):
    import torch
    from nerfshop_amd import runtime as rt, synth
    from oracle import oracle as orc
    ctx = rt.Context(0)
    desc = synth.model_desc(aabb_scale)
    edit = _make_edit(synth, lattice, aabb_scale, rot, copy)
    assert edit.tets.shape[0] == 6 * lattice ** 3 and (edit.local_rotations is None) == (not rot)
    oracles = {}
    for k, (state, verts, pose, op) in enumerate(_states(rt, synth, ctx, desc, edit, aabb_scale)):
        if state != "rested":   # (rested: the pose of "moved" -- the same oracle operator, another batch)
            host = edit if state == "created" else _posed(synth, edit, pose)
            oracles["now"] = orc.Edit(desc, host.tet_mesh_struct(), keepalive=host)
            if aabb_scale == 16 and lattice == 10:
                # the batch reaches cascades with a fine table AND cascades that keep the LUT's own lists (longest list > kFineMaxList = 96)
                longest = [int(np.diff(host.lut_offsets[l * 128 ** 3: (l + 1) * 128 ** 3 + 1].astype(np.int64)).max()) for l in range(5)]
                assert longest[2] <= 96 < longest[3], longest
        c = _batch(synth, edit, verts, aabb_scale, seed=100 * lattice + aabb_scale + k)
        if aabb_scale == 16:   # single waves hold several cascades among the lanes that search a tet (inside the deformed box): the window comes per lane
            world = c[:, :3] * 16 - 7.5
            level = np.ceil(np.log2(np.maximum(np.abs(world - 0.5).max(axis=1) * 2, 1.0))).reshape(-1, 64)
            inside = ((world >= verts.min(0)) & (world <= verts.max(0))).all(axis=1).reshape(-1, 64)
            assert (np.where(inside, level, np.inf).min(axis=1) != np.where(inside, level, -np.inf).max(axis=1)).mean() > 0.5
        ref_c, ref_e = oracles["now"].map_rays(c)
        ref_p, ref_e2 = oracles["now"].map_positions(c[:, :3])
        got_c, got_e, got_p, got_e2 = _gpu_maps(torch, op, c)
        moved = (ref_c[:, :3] != c[:, :3]).any(axis=1)
        assert moved.sum() > N // 8, (state, moved.sum())   # not vacuous: a good share of the batch was carried back by a tet
        if rot:
            assert (ref_c[moved, 4:] != c[moved, 4:]).any(axis=1).mean() > 0.9   # ... and turned by its rotation
        else:
            assert np.array_equal(ref_c[:, 4:], c[:, 4:])
        assert ref_e2.any() and (copy or ref_e.any()) and not (copy and ref_e.any())   # (map_rays honours `copy`, map_positions ignores it)
        assert np.array_equal(got_c.view(np.uint32), ref_c.view(np.uint32)), (state, int((got_c != ref_c).any(axis=1).sum()))
        assert np.array_equal(got_e, ref_e), state
        assert np.array_equal(got_p.view(np.uint32), ref_p.view(np.uint32)), (state, int((got_p != ref_p).any(axis=1).sum()))
        assert np.array_equal(got_e2, ref_e2), state


def test_lego_cage_frame_against_the_oracle(built):
    """a 96 x 64 frame of the bench's lego_cage scene (the render round's own call of the operator, lattice 10) with the frame bars of tests/test_gpu_parity.py"""
    import torch
    from nerfshop_amd import runtime as rt, synth
    from oracle import oracle as orc
    from test_gpu_parity import _compare_frames
    ctx = rt.Context(0)
    desc = synth.model_desc(1)
    params = synth.make_params(desc, sigma_raw=synth.default_sigma_raw(1))
    edit = synth.make_cage_edit(lattice_n=10)
    o_edit = orc.Edit(desc, edit.tet_mesh_struct(), keepalive=edit)
    bitfield = synth.grid_to_bitfield(synth.deformed_density_grid(synth.density_grid(1), desc, o_edit.map_positions, 1))
    o_model = orc.Model(desc, params, bitfield)
    tb = rt.Testbed(ctx, desc, 1)
    tb.nerf_network.set_params(params)
    tb.nerf_network.set_density_bitfield(bitfield)
    tb.add_edit_operator(rt.CageDeformation(ctx, desc, edit))
    p = synth.render_params(96, 64, synth.orbit_camera(30.0))
    frame = torch.zeros((64, 96, 4), device="cuda:0")
    depth = torch.zeros((64, 96), device="cuda:0")
    steps = torch.zeros((64, 96), dtype=torch.int32, device="cuda:0")
    tb.render_with_params(tb.nerf_network, p, frame, depth, steps, None)
    torch.cuda.synchronize()
    ref_frame, ref_depth, ref_steps, _ = o_model.render(p, [o_edit])
    assert (ref_frame[..., 3] > 0.2).mean() > 0.05
    _compare_frames(frame.cpu().numpy(), depth.cpu().numpy(), steps.cpu().numpy(), ref_frame, ref_depth, ref_steps)


def _child(out, aabb_scale, lattice):
    """created and rested state of one operator, through whatever tables this process's knobs leave it"""
    import torch
    from nerfshop_amd import runtime as rt, synth
    ctx = rt.Context(0)
    desc = synth.model_desc(aabb_scale)
    edit = _make_edit(synth, lattice, aabb_scale)
    res = {}
    for k, (state, verts, pose, op) in enumerate(_states(rt, synth, ctx, desc, edit, aabb_scale)):
        if state == "moved":
            continue
        c = _batch(synth, edit, verts, aabb_scale, seed=7 + k)
        got = _gpu_maps(torch, op, c)
        for name, a in zip(("coords", "empty", "pos", "empty_pos"), got):
            res[f"{state}_{name}"] = a
        res[f"{state}_moved"] = np.array([(got[0][:, :3] != c[:, :3]).any(axis=1).sum()])
    np.savez(out, **res)


@pytest.mark.parametrize("aabb_scale,lattice", [(1, 10), (16, 10)])
def test_without_head_words_is_the_same_operator(built, tmp_path, aabb_scale, lattice):
    outs = {}
    for tag, extra in (("heads", {}), ("no_heads", {"NRS_NO_FINE_HEAD": "1"})):
        out = str(tmp_path / f"{tag}.npz")
        env = dict(os.environ, NRS_DEV_KNOBS="1", NRS_FINE_LOG="1", **extra)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), ROOT, out, str(aabb_scale), str(lattice)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        # both runs scan fine lists, built at creation and by the second frame after the move -- with head words in the one, without in the other (the knob took effect,
        # and the run with heads did not fall back silently)
        lines = [ln for ln in r.stderr.splitlines() if ln.startswith("[nrs fine lut]")]
        assert len(lines) == 2 and all(ln.endswith("head words " + ("yes" if tag == "heads" else "no")) for ln in lines), r.stderr[-2000:]
        outs[tag] = np.load(out)
    assert sorted(outs["heads"].files) == sorted(outs["no_heads"].files) and len(outs["heads"].files) == 10
    for key in outs["heads"].files:
        a, b = outs["heads"][key], outs["no_heads"][key]
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b), key
    assert int(outs["heads"]["created_moved"][0]) > N // 8 and int(outs["heads"]["rested_moved"][0]) > N // 8


if __name__ == "__main__":
    sys.path.insert(0, sys.argv[1])
    _child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
