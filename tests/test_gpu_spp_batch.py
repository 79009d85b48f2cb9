"""K samples per pixel of one view in one launch: nrs_render_nerf_spp / nrs_accumulate_spp against the K-call loop they replace.

The yardstick is the unchanged single-frame path -- nrs_render_nerf with spp_index = first + k, nrs_accumulate with sample_count + k -- which the rest of the suite
holds to the oracle; never the batch against itself.  The renderer is deterministic and every schedule is bit-equal to every other
(tests/test_gpu_route_matrix.py), so the bar is equality of bits, compared as uint32 words:

  1. slab k of frame / depth / steps == the single frame of sample first + k, statistics == the sum of the K calls', for K in {1, 2, 5, 8}, a non-zero first index,
     snap_to_pixel_centers off and on, on every family of instantiations, every forced schedule and the automatic one, whole image (173 x 131: partial packets on
     both edges) and the tiles of a 3-rank deal;
  2. every batch render uses slabs that are further apart than one slab is long, with the gaps, a tail guard and the pixels of edge tiles outside the image filled
     with a sentinel: no word outside the K slabs may change;
  3. the fold == K accumulates, for Linear / SRGB / VisPosNeg and sample_count 0 / non-zero;
  4. a batch is ONE dispatch of the render kernel (the library's launch counter);
  5. bad arguments are refused with NRS_ERR_INVALID_ARG and a message that names the argument;
  6. K = 1 is nrs_render_nerf, and a batch leaves the feedback word that sizes the next single-frame launch alone."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_route_matrix import Rigs, SENTINEL, _with, owned_mask, route_on

pytestmark = pytest.mark.gpu

KS = (1, 2, 5, 8)
FIRST = 3           # first spp_index of every batch
WHOLE = (173, 131)
GAP = 37            # pixels between two slabs (sentinel-filled)
TAIL = 4099         # pixels behind the last slab (sentinel-filled)
DEPTH_MODE = 4

# name -> (route of tests/test_gpu_route_matrix.py, render-params fields, extras)
CASES = {
    "noedit": ("R1_noedit", {}, None),
    "cage": ("R2_cage", {}, None),
    "membrane": ("R3_membrane_t0", {}, None),
    "affine": ("R4_affine", {}, None),
    "tcnn_numerics": ("R7_num11_cage", {}, None),
    "extra_dof": ("R2_cage", {"dof": 0.02, "slice_plane_z": 1.2}, None),                        # the aperture draw (pixel_ray_raw)
    "extra_depth_rolling_shutter": ("R2_cage", {"render_mode": DEPTH_MODE, "depth_scale": 0.7}, "rolling_shutter"),   # the rolling-shutter draw
    "rolling_shutter_shade": ("R1_noedit", {}, "rolling_shutter"),                                # ... and on the default kernel
    "envmap": ("R2_cage", {}, "envmap"),
    "gate_aabb16": ("R11_gate_cage", {}, None),
}


@pytest.fixture(scope="module")
def rigs(rig, rig16):
    return Rigs(lego=rig, aabb16=rig16)


def _prepare(rig, p, fields, extra):
    """-> params of the case (and what must stay alive with them)"""
    keep = None
    q = _with(p, **fields)
    if extra == "rolling_shutter":  # the camera moves during the exposure and every ray draws its own time
        q.rolling_shutter[:] = (0.1, 0.2, 0.3, 0.4)
        for i in (9, 10, 11):
            q.camera_matrix1[i] = q.camera_matrix0[i] + 0.02 * (i - 8)
    elif extra == "envmap":
        torch = rig.torch
        g = torch.Generator().manual_seed(5)
        keep = torch.rand((16, 32, 4), generator=g, dtype=torch.float32).to("cuda:0")
        rig.rt.set_camera_extras(q, envmap=keep)
    return q, keep


def _geometry(p):
    W, H, T = p.resolution[0], p.resolution[1], p.tile_size
    if T == 0:
        return (H, W), np.ones((H, W), bool)
    owned, inside, _ = owned_mask(p)
    return (owned, T, T), inside


def loop_render(rig, p, first, k_max, snap):
    """the K-call loop: sample first + k through nrs_render_nerf -> ([K, lead..., 4], [K, lead...], [K, lead...]) as uint32 words, [stats]"""
    torch = rig.torch
    lead, _ = _geometry(p)
    frames, depths, steps, stats = [], [], [], []
    for k in range(k_max):
        q = _with(p, spp_index=first + k, snap_to_pixel_centers=snap)
        f = torch.zeros(lead + (4,), dtype=torch.float32, device="cuda:0")
        d = torch.zeros(lead, dtype=torch.float32, device="cuda:0")
        s = torch.zeros(lead, dtype=torch.int32, device="cuda:0")
        st = rig.testbed.render_with_params(rig.net, q, f, d, s, None, want_stats=True)
        torch.cuda.synchronize()
        frames.append(f.cpu().numpy().view(np.uint32)); depths.append(d.cpu().numpy().view(np.uint32)); steps.append(s.cpu().numpy().view(np.uint32))
        stats.append((st.n_samples, st.n_rays_alive, st.n_rays_hit))
    return np.stack(frames), np.stack(depths), np.stack(steps), stats


def batch_render(rig, p, first, K, snap):
    """one nrs_render_nerf_spp into slabs GAP pixels further apart than they are long, everything around them a sentinel; asserts that no word outside the slabs
    changed -> (frames, depths, steps) as uint32 [K, lead...], stats"""
    torch = rig.torch
    lead, inside = _geometry(p)
    n = int(np.prod(lead))
    stride = n + GAP
    total = K * stride + TAIL
    q = _with(p, spp_index=first, snap_to_pixel_centers=snap)
    host, dev = [], []
    for ch in (4, 1, 1):
        h = np.full((total, ch), SENTINEL, np.uint32)
        for k in range(K):
            slab = h[k * stride:k * stride + n].reshape(lead + (ch,))
            slab[inside] = 0  # the caller clears the frame; depth / steps are written for every pixel inside the image
        host.append(h)
        dev.append(torch.from_numpy(h.view(np.int32).copy()).to("cuda:0"))
    st = rig.testbed.render_spp_with_params(rig.net, q, K, dev[0].view(torch.float32), dev[1].view(torch.float32), dev[2], stride, None, want_stats=True)
    torch.cuda.synchronize()
    out = []
    for b, ch, name in zip(dev, (4, 1, 1), ("frame", "depth", "steps")):
        h = b.cpu().numpy().view(np.uint32)
        guard = np.ones(total, bool)
        slabs = []
        for k in range(K):
            slab = h[k * stride:k * stride + n].reshape(lead + (ch,))
            guard[k * stride:k * stride + n] = False
            outside = slab[~inside]
            assert (outside == SENTINEL).all(), f"{name}, slab {k}: {int((outside != SENTINEL).sum())} words written to pixels outside the image"
            slabs.append(slab if ch > 1 else slab[..., 0])
        assert (h[guard] == SENTINEL).all(), f"{name}: {int((h[guard] != SENTINEL).sum())} words written outside the {K} slabs"
        out.append(np.stack(slabs))
    return out[0], out[1], out[2], (st.n_samples, st.n_rays_alive, st.n_rays_hit)


def assert_batch_is_loop(rig, p, what, ks=KS, snaps=(0, 1)):
    _, inside = _geometry(p)
    n_alive = 0
    for snap in snaps:
        ref = loop_render(rig, p, FIRST, max(ks), snap)
        if not snap:  # the samples differ from one another: the loop is a real yardstick
            assert any(not np.array_equal(ref[0][0], ref[0][k]) for k in range(1, max(ks))), what
        for K in ks:
            got = batch_render(rig, p, FIRST, K, snap)
            for k in range(K):
                for g, r, name in zip(got[:3], ref[:3], ("frame", "depth", "steps")):
                    a, b = g[k][inside], r[k][inside]
                    assert np.array_equal(a, b), f"{what}, snap {snap}, K {K}: {name} of slab {k} differs from nrs_render_nerf(spp_index {FIRST + k}) in {int((a != b).sum())} words"
            want = tuple(sum(s[i] for s in ref[3][:K]) for i in range(3))
            assert got[3] == want, (what, snap, K, got[3], want)
            n_alive += got[3][1]
    return n_alive


@pytest.mark.parametrize("case", list(CASES))
def test_batch_equals_loop(rigs, case):
    route, fields, extra = CASES[case]
    with route_on(rigs, route, size=WHOLE) as (rig, _, p):
        q, keep = _prepare(rig, p, fields, extra)
        assert assert_batch_is_loop(rig, q, case) > 1000
        del keep


@pytest.mark.parametrize("schedule", [1, 2, 4, -1, -2, -3, -4, 0])
def test_batch_equals_loop_on_every_schedule(rigs, schedule):
    with route_on(rigs, "R2_cage", size=WHOLE) as (rig, _, p):
        rig.ctx.set_lane_teams(schedule)
        assert assert_batch_is_loop(rig, p, f"cage, schedule {schedule}") > 1000
        sched = rig.ctx.render_launches()[1]
        if schedule > 0:
            assert sched & 0xff == schedule
        elif schedule == -1:
            assert sched & (1 << 17), "the forced hybrid schedule ran another queue"
        else:
            assert sched & 0xff == 0 and sched & (1 << 16)


@pytest.mark.parametrize("schedule", [0, 1, 2, 4, -3])
def test_batch_equals_loop_on_tiles(rigs, schedule):
    """the tiles of a 3-rank deal (32-pixel tiles, rank r owns tiles r, r + 3, ...): a wrong packet geometry writes past the compact buffer -- the sentinels"""
    with route_on(rigs, "R2_cage", size=WHOLE) as (rig, _, p):
        rig.ctx.set_lane_teams(schedule)
        n = 0
        for rank in range(3):
            q = _with(p, tile_size=32, tile_first=rank, tile_stride=3)
            n += assert_batch_is_loop(rig, q, f"tiles, rank {rank}, schedule {schedule}", ks=(2, 5), snaps=(0,))
        assert n > 1000


def test_batch_equals_loop_extra_on_tiles(rigs):
    with route_on(rigs, "R2_cage", size=WHOLE) as (rig, _, p):
        q, _ = _prepare(rig, p, {"dof": 0.02, "slice_plane_z": 1.2}, None)
        for rank in range(3):
            assert_batch_is_loop(rig, _with(q, tile_size=32, tile_first=rank, tile_stride=3), f"dof tiles, rank {rank}", ks=(5,), snaps=(0,))


@pytest.mark.parametrize("color_space", [0, 1, 2])
@pytest.mark.parametrize("sample_count", [0, 5])
def test_fold_equals_k_accumulates(rig, color_space, sample_count):
    torch = rig.torch
    from nerfshop_amd import _abi
    lib = _abi.load()
    W, H = 173, 131
    n = W * H
    g = torch.Generator().manual_seed(11 + color_space)
    for K, stride in ((1, n), (2, n + GAP), (5, n), (8, n + GAP)):
        slabs = torch.rand((K, stride, 4), generator=g, dtype=torch.float32) * 1.5   # (above 1 and, below, tiny and zero values: both branches of linear_to_srgb)
        slabs[:, ::7] *= 1e-3
        slabs[:, ::13] = 0.0
        slabs = slabs.to("cuda:0")
        start = torch.rand((n, 4), generator=g, dtype=torch.float32).to("cuda:0")
        loop, fold = start.clone(), start.clone()
        for k in range(K):
            _abi.check(lib.nrs_accumulate(rig.ctx.h, None, W, H, slabs[k].data_ptr(), loop.data_ptr(), sample_count + k, color_space))
        _abi.check(lib.nrs_accumulate_spp(rig.ctx.h, None, W, H, slabs.data_ptr(), stride, K, fold.data_ptr(), sample_count, color_space))
        torch.cuda.synchronize()
        a, b = fold.cpu().numpy().view(np.uint32), loop.cpu().numpy().view(np.uint32)
        assert np.array_equal(a, b), f"color space {color_space}, sample_count {sample_count}, K {K}: {int((a != b).sum())} words differ from {K} nrs_accumulate calls"
        if sample_count:
            assert not np.array_equal(b, start.cpu().numpy().view(np.uint32))


def test_render_buffer_accumulate_spp(rig):
    """the harness: Testbed.render_nerf_spp + RenderBuffer.accumulate_spp against the render_nerf + accumulate loop; spp() advances by K"""
    torch, rt = rig.torch, rig.rt
    rig.use_edit(True)
    try:
        W, H, K = 160, 90, 4
        p = rig.scene.params_for(W, H, 60.0)
        args = (tuple(p.focal_length), list(p.camera_matrix0), list(p.camera_matrix1), list(p.rolling_shutter), tuple(p.screen_center), True)
        rig.testbed.snap_to_pixel_centers = False
        a, b = rt.RenderBuffer(W, H, with_steps=True), rt.RenderBuffer(W, H, with_steps=True)
        a.set_spp(2); b.set_spp(2)
        a._accumulate = torch.full((H, W, 4), 0.25, dtype=torch.float32, device="cuda:0"); b._accumulate = a._accumulate.clone()
        for _ in range(K):
            a.clear_frame()
            rig.testbed.render_nerf(rig.net, a, None, *args)
            a.accumulate(rig.ctx)
        frames, depths, steps, _ = rig.testbed.render_nerf_spp(rig.net, b, K, *args)
        assert tuple(frames.shape) == (K, H, W, 4) and tuple(depths.shape) == (K, H, W) and tuple(steps.shape) == (K, H, W)
        acc = b.accumulate_spp(rig.ctx, frames)
        torch.cuda.synchronize()
        assert a.spp() == b.spp() == 2 + K
        assert np.array_equal(acc.cpu().numpy().view(np.uint32), a._accumulate.cpu().numpy().view(np.uint32))
        assert np.array_equal(frames[K - 1].cpu().numpy().view(np.uint32), a.frame_buffer().cpu().numpy().view(np.uint32))
    finally:
        rig.testbed.snap_to_pixel_centers = True
        rig.use_edit(False)


def test_batch_is_one_dispatch(rigs):
    with route_on(rigs, "R2_cage", size=WHOLE) as (rig, _, p):
        n0, _ = rig.ctx.render_launches()
        loop_render(rig, p, FIRST, 8, 0)
        n1, sched = rig.ctx.render_launches()
        assert n1 - n0 == 8 and not sched & (1 << 18)
        batch_render(rig, p, FIRST, 8, 0)
        n2, sched = rig.ctx.render_launches()
        assert n2 - n1 == 1, f"a batch of 8 samples took {n2 - n1} render-kernel dispatches"
        assert sched & (1 << 18)
        batch_render(rig, p, FIRST, 1, 0)   # K = 1 runs the single frame's kernel
        n3, sched = rig.ctx.render_launches()
        assert n3 - n2 == 1 and not sched & (1 << 18)


def test_arguments_are_checked(rigs):
    from nerfshop_amd._abi import NrsError, SPP_BATCH_MAX
    with route_on(rigs, "R2_cage", size=WHOLE) as (rig, _, p):
        torch = rig.torch
        W, H = WHOLE
        n = W * H
        frames = torch.zeros((2, H, W, 4), dtype=torch.float32, device="cuda:0")
        depths = torch.zeros((2, H, W), dtype=torch.float32, device="cuda:0")
        n0 = rig.ctx.render_launches()[0]

        def refused(word, p=p, K=2, frames=frames, depths=depths, stride=n):
            with pytest.raises(NrsError) as e:
                rig.testbed.render_spp_with_params(rig.net, p, K, frames, depths, None, stride)
            assert "nrs error -1:" in str(e.value) and word in str(e.value), str(e.value)   # NRS_ERR_INVALID_ARG

        refused("spp_count", K=0)
        refused("NRS_SPP_BATCH_MAX", K=SPP_BATCH_MAX + 1)
        refused("slab_stride_pixels", stride=n - 1)
        refused("slab_stride_pixels", stride=0)
        refused("slab_stride_pixels", stride=(1 << 32) // 2)
        refused("Slice", p=_with(p, render_mode=9, slice_plane_z=1.3))
        refused("resolution", p=_with(p, resolution=(C.c_int32 * 2)(8200, 16)), stride=8200 * 16)
        tiled = _with(p, tile_size=32, tile_first=0, tile_stride=3)
        owned = owned_mask(tiled)[0]
        refused("slab_stride_pixels", p=tiled, stride=owned * 32 * 32 - 1)
        lib = rig.ctx.lib
        arr = (C.c_void_p * 1)(rig.op.h)
        for fr, dp in ((None, depths.data_ptr()), (frames.data_ptr(), None)):
            assert lib.nrs_render_nerf_spp(rig.net.h, C.byref(p), arr, 1, 2, fr, dp, None, n, None, None) == -1
            assert b"d_frames" in lib.nrs_last_error()
        # the fold's
        acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
        for args, word in (((frames.data_ptr(), n, 0, acc.data_ptr(), 0, 0), b"spp_count"), ((frames.data_ptr(), n, SPP_BATCH_MAX + 1, acc.data_ptr(), 0, 0), b"NRS_SPP_BATCH_MAX"),
                           ((frames.data_ptr(), n - 1, 2, acc.data_ptr(), 0, 0), b"slab_stride_pixels"), ((None, n, 2, acc.data_ptr(), 0, 0), b"d_frames"),
                           ((frames.data_ptr(), n, 2, None, 0, 0), b"d_accumulate"), ((frames.data_ptr(), n, 2, acc.data_ptr(), 0, 3), b"color_space")):
            assert lib.nrs_accumulate_spp(rig.ctx.h, None, W, H, *args) == -1
            assert word in lib.nrs_last_error(), lib.nrs_last_error()
        torch.cuda.synchronize()
        assert rig.ctx.render_launches()[0] == n0, "a refused call launched a kernel"
        assert not frames.any() and not depths.any()


def _looking_away(p):
    q = _with(p)
    for m in (q.camera_matrix0, q.camera_matrix1):
        for i in (0, 1, 2, 6, 7, 8):   # the x and the view axis turn round: the scene lies behind the camera
            m[i] = -m[i]
    return q


def test_batch_leaves_the_feedback_word_alone(rig):
    """The automatic schedule sizes a launch from the share of the pixels that became rays in the last finished launch (at 1280 x 720 that share decides how many
    lanes stand on a pixel during the fill).  A batch of a view that hits nothing, between two single frames of a view that does: the second frame takes the route
    and gives the bits it takes and gives without the batch."""
    torch = rig.torch
    rig.use_edit(True)
    try:
        W, H = 1280, 720
        p = rig.scene.params_for(W, H, 60.0)
        first = rig.render(p)
        second = rig.render(p)                  # sized by the first frame's feedback
        route = rig.ctx.render_launches()[1]
        frames = torch.zeros((2, H, W, 4), dtype=torch.float32, device="cuda:0")
        depths = torch.zeros((2, H, W), dtype=torch.float32, device="cuda:0")
        st = rig.testbed.render_spp_with_params(rig.net, _looking_away(p), 2, frames, depths, None, W * H, None, want_stats=True)
        assert st.n_rays_hit == 0 and st.n_samples == 0
        third = rig.render(p)
        route3 = rig.ctx.render_launches()[1]
        # what a single frame of that view does to the next frame's route (where it differs, a batch that wrote the word would have shown above)
        rig.render(_looking_away(p))
        rig.render(p)
        control = rig.ctx.render_launches()[1]
        print(f"[feedback] hit share {first[3].n_rays_alive / (W * H):.3f}: route {route:#x}, after the batch {route3:#x}, after a single frame that hits nothing {control:#x}")
        rig.render(p)
        assert control != route, "the control cannot see a written feedback word at this resolution"
        assert route3 == route, "the frame after a batch took another route: the batch wrote the feedback word"
        for a, b in zip(second[:3], third[:3]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    finally:
        rig.use_edit(False)
