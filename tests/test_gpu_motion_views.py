"""A view per sample in one launch: nrs_render_nerf_spp_views against the K-call loop it replaces, and render_to_cpu's moving camera on top of it.

The yardstick is always the unchanged single-frame path -- nrs_render_nerf, one call per sample, with that sample's view written into the params -- never the
views batch against itself.  The renderer is deterministic, so the bar is equality of bits, compared as uint32 words.

The views of a batch really differ (make_views): sample k is turned about the scene by a few degrees and shifted, its end-of-shutter camera differs from its
start camera, its focal length is scaled by 1 + 0.03 k and, where the case has an aperture, dof and focus distance differ per sample; the yardstick's slabs are
asserted to differ from one another with snap_to_pixel_centers = 1, where jitter cannot be the reason.

  1. slab k == the single frame of view k, statistics == the sum, on every case of tests/test_gpu_spp_batch.py and a network with light directions;
  2. the cage case on every forced schedule and the automatic one (the hand-over and re-teaming paths move a ray's sample), and on the tiles of a 3-rank deal;
  3. slabs GAP pixels further apart than they are long, sentinels everywhere else: no word outside the K slabs changes (batch_views checks it on every call);
  4. K views equal to the params' own == nrs_render_nerf_spp, h_views = NULL == the same, K = 1 with a view == nrs_render_nerf of that view;
  5. a views batch is one dispatch with the schedule word's views bit set (a still batch: clear), and it leaves the hit-share feedback word alone;
  6. refusals name the argument;
  7. render_to_cpu with a moving camera == the loop nrs_motion_views -> nrs_render_nerf -> nrs_accumulate -> nrs_tonemap; with the new arguments at their defaults
     it is the still call."""
import ctypes as C
import json

import numpy as np
import pytest

from test_gpu_route_matrix import Rigs, SENTINEL, _with, route_on
from test_gpu_spp_batch import CASES, FIRST, GAP, KS, TAIL, WHOLE, _geometry, _looking_away, _prepare, batch_render

pytestmark = pytest.mark.gpu

VIEWS_BIT, BATCH_BIT = 1 << 19, 1 << 18


@pytest.fixture(scope="module")
def rigs(rig, rig16):
    return Rigs(lego=rig, aabb16=rig16)


def _turned(cam, degrees, shift, centre):
    """the 3x4 column-major camera turned about the vertical axis through `centre` and shifted"""
    a = np.deg2rad(degrees)
    rot = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    m = np.asarray(list(cam), np.float64).reshape(4, 3).T   # [3, 4]
    out = np.empty((3, 4))
    out[:, :3] = rot @ m[:, :3]
    out[:, 3] = rot @ (m[:, 3] - centre) + centre + shift
    return [float(v) for v in out.T.reshape(-1).astype(np.float32)]


def make_views(p, K, aperture, scene_scale=1.0):
    from nerfshop_amd._abi import SampleView
    centre = np.full(3, 0.5)
    views = (SampleView * K)()
    for k in range(K):
        v = views[k]
        v.camera_matrix0[:] = _turned(p.camera_matrix0, 2.5 * k, np.array([0.004, -0.003, 0.002]) * k * scene_scale, centre)
        v.camera_matrix1[:] = _turned(p.camera_matrix1, 2.5 * k + 0.8, np.array([0.004, -0.003, 0.002]) * (k + 0.5) * scene_scale, centre)
        v.focal_length[:] = [float(np.float32(f * (1.0 + 0.03 * k))) for f in p.focal_length]
        v.dof = p.dof * (1.0 + 0.25 * k) if aperture else p.dof
        v.slice_plane_z = p.slice_plane_z + 0.05 * k if aperture else p.slice_plane_z
        assert list(v.camera_matrix0) != list(v.camera_matrix1)
    return views


def with_view(p, v, **fields):
    q = _with(p, **fields)
    q.camera_matrix0[:] = list(v.camera_matrix0)
    q.camera_matrix1[:] = list(v.camera_matrix1)
    q.focal_length[:] = list(v.focal_length)
    q.dof, q.slice_plane_z = v.dof, v.slice_plane_z
    return q


def loop_views(rig, p, views, first, snap):
    """the yardstick: sample first + k through nrs_render_nerf with view k written into the params"""
    torch = rig.torch
    lead, _ = _geometry(p)
    frames, depths, steps, stats = [], [], [], []
    for k in range(len(views)):
        q = with_view(p, views[k], spp_index=first + k, snap_to_pixel_centers=snap)
        f = torch.zeros(lead + (4,), dtype=torch.float32, device="cuda:0")
        d = torch.zeros(lead, dtype=torch.float32, device="cuda:0")
        s = torch.zeros(lead, dtype=torch.int32, device="cuda:0")
        st = rig.testbed.render_with_params(rig.net, q, f, d, s, None, want_stats=True)
        torch.cuda.synchronize()
        frames.append(f.cpu().numpy().view(np.uint32)); depths.append(d.cpu().numpy().view(np.uint32)); steps.append(s.cpu().numpy().view(np.uint32))
        stats.append((st.n_samples, st.n_rays_alive, st.n_rays_hit))
    return np.stack(frames), np.stack(depths), np.stack(steps), stats


def batch_views(rig, p, views, first, K, snap, null_views=False):
    """one nrs_render_nerf_spp_views of views[:K] into slabs GAP pixels further apart than they are long, everything around them a sentinel; asserts that no word
    outside the slabs changed -> (frames, depths, steps) as uint32 [K, lead...], stats"""
    from nerfshop_amd._abi import SampleView
    torch = rig.torch
    lead, inside = _geometry(p)
    n = int(np.prod(lead))
    stride = n + GAP
    total = K * stride + TAIL
    q = _with(p, spp_index=first, snap_to_pixel_centers=snap)
    dev = []
    for ch in (4, 1, 1):
        h = np.full((total, ch), SENTINEL, np.uint32)
        for k in range(K):
            h[k * stride:k * stride + n].reshape(lead + (ch,))[inside] = 0
        dev.append(torch.from_numpy(h.view(np.int32).copy()).to("cuda:0"))
    vs = None if null_views else (SampleView * K)(*[views[k] for k in range(K)])
    st = rig.testbed.render_spp_with_views(rig.net, q, vs, dev[0].view(torch.float32), dev[1].view(torch.float32), dev[2], stride, None, want_stats=True, spp_count=K)
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


def assert_views_are_loop(rig, p, what, aperture=False, ks=KS, snaps=(0, 1), scene_scale=1.0):
    _, inside = _geometry(p)
    views = make_views(p, max(ks), aperture, scene_scale)
    n_alive = 0
    for snap in snaps:
        ref = loop_views(rig, p, views, FIRST, snap)
        if snap and max(ks) > 1:   # without jitter only the view can make two samples differ: every slab of the yardstick is its own picture
            for k in range(1, max(ks)):
                assert not np.array_equal(ref[0][0][inside], ref[0][k][inside]) and not np.array_equal(ref[0][k - 1][inside], ref[0][k][inside]), (what, k)
        for K in ks:
            got = batch_views(rig, p, views, FIRST, K, snap)
            for k in range(K):
                for g, r, name in zip(got[:3], ref[:3], ("frame", "depth", "steps")):
                    a, b = g[k][inside], r[k][inside]
                    assert np.array_equal(a, b), f"{what}, snap {snap}, K {K}: {name} of slab {k} differs from nrs_render_nerf of view {k} in {int((a != b).sum())} words"
            want = tuple(sum(s[i] for s in ref[3][:K]) for i in range(3))
            assert got[3] == want, (what, snap, K, got[3], want)
            n_alive += got[3][1]
    return n_alive


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_views_equal_loop(rigs, case):
    route, fields, extra = CASES[case]
    with route_on(rigs, route, size=WHOLE) as (rig, _, p):
        q, keep = _prepare(rig, p, fields, extra)
        scale = 6.0 if rig.scene.aabb_scale != 1 else 1.0
        assert assert_views_are_loop(rig, q, case, aperture="dof" in fields, scene_scale=scale) > 1000
        del keep


def test_views_equal_loop_light_dirs(rig):
    """a network trained with light directions: its LIGHT twin of the default kernel, and (Depth mode) its catch-all"""
    from test_gpu_light_dirs import Fold, LightRig, _load_fold
    lrig, fold = LightRig(rig), Fold(rig.scene)
    _load_fold(lrig, fold, 1)
    p = rig.scene.params_for(WHOLE[0], WHOLE[1], 60.0)
    assert assert_views_are_loop(lrig, p, "light", ks=(2, 5)) > 1000
    assert assert_views_are_loop(lrig, _with(p, render_mode=4, depth_scale=0.7), "light, depth", ks=(5,), snaps=(1,)) > 500


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", [1, 2, 4, -1, -2, -3, -4, 0])
def test_views_equal_loop_on_every_schedule(rigs, schedule):
    with route_on(rigs, "R2_cage", size=WHOLE) as (rig, _, p):
        rig.ctx.set_lane_teams(schedule)
        assert assert_views_are_loop(rig, p, f"cage, schedule {schedule}") > 1000
        sched = rig.ctx.render_launches()[1]
        assert sched & VIEWS_BIT and sched & BATCH_BIT
        if schedule > 0:
            assert sched & 0xff == schedule
        elif schedule == -1:
            assert sched & (1 << 17), "the forced hybrid schedule ran another queue"
        else:
            assert sched & 0xff == 0 and sched & (1 << 16)


@pytest.mark.parametrize("schedule", [0, 1, 4, -3])
def test_views_equal_loop_on_tiles(rigs, schedule):
    """the tiles of a 3-rank deal (32-pixel tiles): a ray's sample is its output index over the slab stride, and a tiled slab is indexed by owned tile"""
    with route_on(rigs, "R2_cage", size=WHOLE) as (rig, _, p):
        rig.ctx.set_lane_teams(schedule)
        n = 0
        for rank in range(3):
            q = _with(p, tile_size=32, tile_first=rank, tile_stride=3)
            n += assert_views_are_loop(rig, q, f"tiles, rank {rank}, schedule {schedule}", snaps=(1,))
        assert n > 1000


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------------------
def test_equal_views_are_the_still_batch(rigs):
    from nerfshop_amd._abi import SampleView
    with route_on(rigs, "R2_cage", size=WHOLE) as (rig, _, p):
        q, _ = _prepare(rig, p, {}, "rolling_shutter")
        _, inside = _geometry(q)
        K = 5
        own = SampleView()
        own.camera_matrix0[:] = list(q.camera_matrix0); own.camera_matrix1[:] = list(q.camera_matrix1); own.focal_length[:] = list(q.focal_length)
        own.dof, own.slice_plane_z = q.dof, q.slice_plane_z
        still = batch_render(rig, q, FIRST, K, 0)
        n0 = rig.ctx.render_launches()[0]
        same = batch_views(rig, q, [own] * K, FIRST, K, 0)
        assert rig.ctx.render_launches()[1] & VIEWS_BIT
        null = batch_views(rig, q, None, FIRST, K, 0, null_views=True)
        sched = rig.ctx.render_launches()[1]
        assert sched & BATCH_BIT and not sched & VIEWS_BIT, "h_views = NULL is nrs_render_nerf_spp"
        assert rig.ctx.render_launches()[0] - n0 == 2
        for got, what in ((same, "K equal views"), (null, "h_views = NULL")):
            for g, r in zip(got[:3], still[:3]):
                assert np.array_equal(g[:, inside], r[:, inside]), what
            assert got[3] == still[3], what
        # K = 1 with a view: the single frame's kernel, that view
        views = make_views(q, 2, False)
        one = batch_views(rig, q, [views[1]], FIRST, 1, 0)
        sched = rig.ctx.render_launches()[1]
        assert not sched & BATCH_BIT and not sched & VIEWS_BIT
        ref = loop_views(rig, q, [views[1]], FIRST, 0)
        for g, r in zip(one[:3], ref[:3]):
            assert np.array_equal(g[0][inside], r[0][inside])
        assert one[3] == ref[3][0]


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------------------
def test_views_batch_is_one_dispatch(rigs):
    with route_on(rigs, "R2_cage", size=WHOLE) as (rig, _, p):
        views = make_views(p, 8, False)
        n0, _ = rig.ctx.render_launches()
        batch_render(rig, p, FIRST, 8, 0)
        n1, sched = rig.ctx.render_launches()
        assert n1 - n0 == 1 and sched & BATCH_BIT and not sched & VIEWS_BIT
        batch_views(rig, p, views, FIRST, 8, 0)
        n2, sched = rig.ctx.render_launches()
        assert n2 - n1 == 1, f"a views batch of 8 samples took {n2 - n1} render-kernel dispatches"
        assert sched & BATCH_BIT and sched & VIEWS_BIT


def test_views_batch_leaves_the_feedback_word_alone(rig):
    """as tests/test_gpu_spp_batch.py test_batch_leaves_the_feedback_word_alone: a views batch that hits nothing, between two single frames of a view that does"""
    torch = rig.torch
    rig.use_edit(True)
    try:
        W, H = 1280, 720
        p = rig.scene.params_for(W, H, 60.0)
        rig.render(p)
        second = rig.render(p)
        route = rig.ctx.render_launches()[1]
        frames = torch.zeros((2, H, W, 4), dtype=torch.float32, device="cuda:0")
        depths = torch.zeros((2, H, W), dtype=torch.float32, device="cuda:0")
        away = _looking_away(p)
        views = make_views(away, 2, False)
        st = rig.testbed.render_spp_with_views(rig.net, p, views, frames, depths, None, W * H, None, want_stats=True)
        assert st.n_rays_hit == 0 and st.n_samples == 0
        assert rig.ctx.render_launches()[1] & VIEWS_BIT
        third = rig.render(p)
        route3 = rig.ctx.render_launches()[1]
        rig.render(away)
        rig.render(p)
        control = rig.ctx.render_launches()[1]
        rig.render(p)
        assert control != route, "the control cannot see a written feedback word at this resolution"
        assert route3 == route, "the frame after a views batch took another route: the batch wrote the feedback word"
        for a, b in zip(second[:3], third[:3]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    finally:
        rig.use_edit(False)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------------------
def test_view_arguments_are_checked(rigs):
    from nerfshop_amd._abi import NrsError, SPP_BATCH_MAX, SampleView
    with route_on(rigs, "R2_cage", size=WHOLE) as (rig, _, p):
        torch = rig.torch
        W, H = WHOLE
        n = W * H
        frames = torch.zeros((2, H, W, 4), dtype=torch.float32, device="cuda:0")
        depths = torch.zeros((2, H, W), dtype=torch.float32, device="cuda:0")
        n0 = rig.ctx.render_launches()[0]
        good = make_views(p, 2, False)

        def refused(word, views=good, p=p, K=None, stride=n):
            with pytest.raises(NrsError) as e:
                rig.testbed.render_spp_with_views(rig.net, p, views, frames, depths, None, stride, spp_count=K)
            assert "nrs error -1:" in str(e.value) and word in str(e.value), str(e.value)   # NRS_ERR_INVALID_ARG

        def bad(k, field, index, value):
            vs = (SampleView * 2)(good[0], good[1])
            if index is None:
                setattr(vs[k], field, value)
            else:
                getattr(vs[k], field)[index] = value
            return vs

        refused("h_views[1].camera_matrix0", bad(1, "camera_matrix0", 7, float("nan")))
        refused("h_views[0].camera_matrix1", bad(0, "camera_matrix1", 11, float("inf")))
        refused("h_views[1].focal_length", bad(1, "focal_length", 0, 0.0))
        refused("h_views[0].focal_length", bad(0, "focal_length", 1, -3.0))
        refused("h_views[1].dof", bad(1, "dof", None, float("nan")))
        refused("h_views[0].slice_plane_z", bad(0, "slice_plane_z", None, float("inf")))
        lens = bad(1, "dof", None, 0.1)
        lens[1].slice_plane_z = 0.0
        refused("h_views[1]", lens)   # an aperture without a focus distance, as the single frame refuses it
        refused("spp_count", K=0)
        big = (SampleView * (SPP_BATCH_MAX + 1))(*([good[0]] * (SPP_BATCH_MAX + 1)))
        refused("NRS_SPP_BATCH_MAX", views=big, K=SPP_BATCH_MAX + 1)
        refused("slab_stride_pixels", stride=n - 1)
        refused("Slice", p=_with(p, render_mode=9, slice_plane_z=1.3))
        torch.cuda.synchronize()
        assert rig.ctx.render_launches()[0] == n0, "a refused call launched a kernel"
        assert not frames.any() and not depths.any()


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------------------
def _reference_frame(rig, W, H, spp, views, focal, linear, fmt):
    """nrs_render_nerf per sample with its view -> nrs_accumulate -> nrs_tonemap"""
    rt, tb = rig.rt, rig.testbed
    buf = rt.RenderBuffer(W, H)
    buf._accumulate = None
    for i in range(spp):
        buf.clear_frame()
        p = tb.make_params(buf, focal, views[i].camera_matrix0, views[i].camera_matrix1, (0.0, 0.0, 0.0, 0.0), (0.5, 0.5), True)
        p = with_view(p, views[i])
        tb.render_with_params(rig.net, p, buf.frame_buffer(), buf.depth_buffer())
        buf.accumulate(rig.ctx)
    out = buf.tonemap(rig.ctx, 0.0, (0.0, 0.0, 0.0, 0.0), 0 if linear else 1, fmt)
    rig.torch.cuda.synchronize()
    return out.cpu().numpy()


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_render_to_cpu_moving_camera(rig, tmp_path):
    from nerfshop_amd._abi import CameraKeyframe, SampleView
    tb = rig.testbed
    rig.use_edit(True)
    saved = (tb.snap_to_pixel_centers, tb.dof, tb.slice_plane_z, tb.scale, tb.fov, tb.camera_path, tb.m_camera, tb.m_smoothed_camera)
    try:
        tb.snap_to_pixel_centers = False
        W, H, spp = 160, 90, 5
        p = rig.scene.params_for(W, H, 60.0)
        focal, cam0 = tuple(p.focal_length), list(p.camera_matrix0)
        cam1 = _turned(cam0, 4.0, np.array([0.01, 0.0, -0.01]), np.full(3, 0.5))
        base = SampleView()
        base.focal_length[:] = focal
        base.dof, base.slice_plane_z = tb.dof, tb.slice_plane_z + tb.scale

        # the new arguments at their defaults: the still call (camera_matrix1 is the params' second camera, as before)
        still = tb.render_to_cpu(rig.net, W, H, spp, False, focal, cam0, cam1)
        own = SampleView()
        own.camera_matrix0[:] = cam0; own.camera_matrix1[:] = cam1; own.focal_length[:] = focal
        own.dof, own.slice_plane_z = base.dof, base.slice_plane_z
        assert _same_bits(still, _reference_frame(rig, W, H, spp, [own] * spp, focal, False, "rgba32f"))

        # camera0 -> camera1 over half of the frame time
        views = tb.motion_views(cam0, cam1, 0.5, spp, 0, spp, (W, H), -1.0, -1.0, base)
        assert list(views[0].camera_matrix0) == cam0 and list(views[4].camera_matrix1) != list(views[0].camera_matrix1)
        for fmt in ("rgba32f", "rgba8"):
            n0 = rig.ctx.render_launches()[0]
            got = tb.render_to_cpu(rig.net, W, H, spp, False, focal, cam0, cam1, fmt=fmt, shutter_fraction=0.5)
            assert rig.ctx.render_launches()[0] - n0 == 1 and rig.ctx.render_launches()[1] & VIEWS_BIT
            assert _same_bits(got, _reference_frame(rig, W, H, spp, views, focal, False, fmt)), fmt
            assert tb.m_smoothed_camera == cam1
            if fmt == "rgba32f":
                assert not _same_bits(got, still), "the moving camera rendered the still frame"

        # a 4-keyframe path: the frame runs from the last frame's end camera to the path's camera at end_time; fov, dof and focus plane follow the path per sample
        keys = []
        for i in range(4):
            k = CameraKeyframe()
            m = (C.c_float * 12)(*_turned(cam0, 6.0 * i, np.array([0.01, 0.005, 0.0]) * i, np.full(3, 0.5)))
            assert rig.ctx.lib.nrs_camera_keyframe_from_matrix(C.byref(m), 0.1 * i, 1.0 + 0.05 * i, 45.0 + 3.0 * i, 0.004 * i, C.byref(k)) == 0
            keys.append(k)
        path = tmp_path / "path.json"
        path.write_text(json.dumps({"time": 0.0, "path": [{"R": [float(v) for v in k.R], "T": [float(v) for v in k.T], "slice": float(k.slice), "scale": float(k.scale),
                                                            "fov": float(k.fov), "dof": float(k.dof)} for k in keys]}))
        assert tb.load_camera_path(str(path)) == 4
        start_cam = list(tb.m_smoothed_camera)
        tb.set_camera_from_time(0.3)
        end_cam = list(tb.m_camera)   # (camera smoothing is off: the smoothed camera is the path's)
        views = tb.motion_views(start_cam, end_cam, 0.5, spp, 0, spp, (W, H), 0.25, 0.3, base)
        assert len({v.focal_length[0] for v in views}) == spp and len({v.dof for v in views}) == spp and views[0].dof != 0.0
        for fmt in ("rgba32f", "rgba8"):
            tb.m_smoothed_camera = list(start_cam)
            got = tb.render_to_cpu(rig.net, W, H, spp, False, focal, cam0, fmt=fmt, start_time=0.25, end_time=0.3, shutter_fraction=0.5)
            assert _same_bits(got, _reference_frame(rig, W, H, spp, views, focal, False, fmt)), fmt
            assert tb.m_smoothed_camera == end_cam
    finally:
        tb.snap_to_pixel_centers, tb.dof, tb.slice_plane_z, tb.scale, tb.fov, tb.camera_path, tb.m_camera, tb.m_smoothed_camera = saved
        rig.use_edit(False)


def test_render_to_cpu_full_shutter_and_camera_smoothing(rig):
    """motion_blur=True asks for the blur between two cameras at the reference's default shutter of 1.0, where the default (None) keeps the still call; and with
    camera_smoothing the frame ends on apply_camera_smoothing's camera (testbed.cu:2086-2093: log_space_lerp(smoothed, camera, 1 - 0.02^(1 / fps))), not on the target"""
    from nerfshop_amd._abi import SampleView
    tb = rig.testbed
    rig.use_edit(True)
    saved = (tb.snap_to_pixel_centers, tb.camera_path, tb.m_camera, tb.m_smoothed_camera, tb.camera_smoothing)
    try:
        tb.snap_to_pixel_centers = False
        tb.camera_path = []
        W, H, spp = 160, 90, 3
        p = rig.scene.params_for(W, H, 60.0)
        focal, cam0 = tuple(p.focal_length), list(p.camera_matrix0)
        cam1 = _turned(cam0, 4.0, np.array([0.01, 0.0, -0.01]), np.full(3, 0.5))
        base = SampleView()
        base.focal_length[:] = focal
        base.dof, base.slice_plane_z = tb.dof, tb.slice_plane_z + tb.scale

        own = SampleView()
        own.camera_matrix0[:] = cam0; own.camera_matrix1[:] = cam1; own.focal_length[:] = focal
        own.dof, own.slice_plane_z = base.dof, base.slice_plane_z
        still = _reference_frame(rig, W, H, spp, [own] * spp, focal, False, "rgba32f")
        assert _same_bits(tb.render_to_cpu(rig.net, W, H, spp, False, focal, cam0, cam1, shutter_fraction=1.0), still)
        assert _same_bits(tb.render_to_cpu(rig.net, W, H, spp, False, focal, cam0, cam1, shutter_fraction=0.5, motion_blur=False), still)
        views = tb.motion_views(cam0, cam1, 1.0, spp, 0, spp, (W, H), -1.0, -1.0, base)
        assert np.abs(np.array(views[spp - 1].camera_matrix1, np.float64) - np.array(cam1, np.float64)).max() <= 2.0 ** -23   # (t = 1 gives `end` within one float rounding)
        got = tb.render_to_cpu(rig.net, W, H, spp, False, focal, cam0, cam1, shutter_fraction=1.0, motion_blur=True)
        assert rig.ctx.render_launches()[1] & VIEWS_BIT
        assert _same_bits(got, _reference_frame(rig, W, H, spp, views, focal, False, "rgba32f")) and not _same_bits(got, still)

        # start_time >= 0 without keyframes, smoothing on: from the last frame's end camera (cam0 here) towards camera_matrix1, as far as one frame time of smoothing goes
        tb.camera_smoothing = True
        tb.m_smoothed_camera = list(cam0)
        fps = 24.0
        decay = np.float32(0.02) ** np.float32((1000.0 / fps) / 1000.0)
        end_cam = tb.log_space_lerp(cam0, cam1, float(np.float32(1.0) - np.float32(decay)))
        assert end_cam != cam1 and end_cam != cam0
        views = tb.motion_views(cam0, end_cam, 0.5, spp, 0, spp, (W, H), -1.0, -1.0, base)
        got = tb.render_to_cpu(rig.net, W, H, spp, False, focal, cam0, cam1, start_time=0.5, fps=fps, shutter_fraction=0.5)
        assert _same_bits(got, _reference_frame(rig, W, H, spp, views, focal, False, "rgba32f"))
        assert tb.m_smoothed_camera == end_cam and tb.m_camera == cam1
    finally:
        tb.snap_to_pixel_centers, tb.camera_path, tb.m_camera, tb.m_smoothed_camera, tb.camera_smoothing = saved
        rig.use_edit(False)
