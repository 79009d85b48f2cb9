"""The dataset on the GPU against the twins of tests/dataset_ref.py: image conversion, pixel rays and their targets, masked pixels, the hand-over to the sample
generator, mark_untrained, refusals and states, and Trainer.fit end to end.

What is a single IEEE operation on exact draws (pixels, jitter, targets, backgrounds, the f32 / f16 image formats) is compared bit for bit with the float32 twin.  Ray
origins and directions are judged against the float64 twin in units of 2^-23 (directions are unit length; origins relative to their norm); the bar is four times the
worst error of the float32 twin on the same inputs, as the ray-loss tests set theirs.  The RGBA8 conversion's bar comes from the reference arithmetic itself
(tests/test_dataset_host.py::test_conversion_bar_on_the_cpu): no element more than one fp16 step from the float64 twin, at most 0.1 % different at all, alpha exact.
The figures measured on an MI355X are in profiles/dataset_rays.md."""
import math

import numpy as np
import pytest
import torch

import dataset_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 1337
UNIT = 2.0 ** -23


@pytest.fixture(scope="module")
def ctx(built):
    from nerfshop_amd import runtime
    return runtime.Context(0)


@pytest.fixture(scope="module")
def desc14():
    from nerfshop_amd import synth
    return synth.model_desc(log2_hashmap_size=14)


@pytest.fixture(scope="module")
def full_network(ctx, desc14):
    """a network whose every cell is occupied: the sample generator needs nothing else"""
    from nerfshop_amd import _abi, runtime
    net = runtime.NerfNetwork(ctx, desc14, cell_cache_bytes=0)
    net.set_density_bitfield(np.full(_abi.BITFIELD_BYTES, 255, np.uint8))
    return net


def orbit_record(azimuth, width, mode=0, params=(), moving=False, pp=(0.5, 0.5), rs=(0.0, 0.0, 0.0, 0.0), focal_ratio=1.0):
    """a camera on synth's orbit, looking at the unit box; `moving`: the end transform is the orbit's next position"""
    from nerfshop_amd import synth
    start = np.asarray(synth.orbit_camera(azimuth), np.float32).reshape(4, 3).T
    end = np.asarray(synth.orbit_camera(azimuth + 7.0, 33.0), np.float32).reshape(4, 3).T if moving else start
    focal = 0.5 * width / math.tan(0.5 * synth.CAMERA_ANGLE_X)
    return ref.camera_record(start, end, (focal, focal * focal_ratio), pp, rs, mode, params)


def make_dataset(ctx, cams, images):
    from nerfshop_amd import runtime
    n, H, W = images.shape[:3]
    ds = runtime.Dataset(ctx, n, W, H)
    for k in range(n):
        ds.set_image(k, images[k])
        ds.set_camera(k, ref.to_struct(cams[k]))
    return ds


def random_images(n, W, H, seed=3):
    return np.random.default_rng(seed).random((n, H, W, 4)).astype(np.float16)


def gpu_rays(ds, n_rays, total=0, snap=True, random_bg=True):
    out = ds.rays(n_rays, total, ref.rng_of(SEED), snap=snap, random_bg=random_bg)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in out]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all()


# ---- conversion -------------------------------------------------------------------------------------------------------------------------------------------------
def test_conversion(ctx):
    from nerfshop_amd import _abi, runtime
    img = ref.all_pairs_image()
    want32, want64 = ref.from_rgba8_32(img), ref.from_rgba8_64(img)
    ds = runtime.Dataset(ctx, 3, 256, 256)
    ds.set_image(0, img)
    got = ds.get_image(0)
    steps = ref.half_steps(got, want64)
    share = float((steps > 0).mean())
    print(f"RGBA8 against from_rgba8_64: {int((steps > 0).sum())} of {steps.size} elements differ ({100 * share:.4f} %), worst {int(steps.max())} fp16 step; "
          f"against from_rgba8_32: {int((ref.half_steps(got, want32) > 0).sum())} differ")
    assert steps.max() <= 1 and share <= 0.001
    assert (got[..., 3].view(np.uint16) == want64[..., 3].view(np.uint16)).all(), "alpha is exact"
    # the same pixels through the two linear formats: bit-equal to the twin (a rounding of a float, a copy); from a device tensor as well
    lin = want64.astype(np.float32) * np.float32(1.0009765625) + np.float32(3e-8)   # floats that are not on the fp16 grid
    ds.set_image(1, lin)
    ds.set_image(2, want32)
    assert (ds.get_image(1).view(np.uint16) == lin.astype(np.float16).view(np.uint16)).all()
    assert (ds.get_image(2).view(np.uint16) == want32.view(np.uint16)).all()
    ds.set_image(2, torch.from_numpy(lin).to(DEV))
    ds.set_image(1, torch.from_numpy(img).to(DEV))
    assert (ds.get_image(2).view(np.uint16) == lin.astype(np.float16).view(np.uint16)).all()
    assert (ds.get_image(1).view(np.uint16) == got.view(np.uint16)).all()
    # white / black transparent and a mask colour on chosen pixels: exact
    small = np.random.default_rng(8).integers(1, 255, (3, 5, 4), dtype=np.uint8)
    small[0, 0], small[0, 1], small[1, 2], small[2, 4], small[2, 3] = (255, 255, 255, 200), (0, 0, 0, 77), (9, 8, 7, 6), (255, 255, 254, 200), (0, 1, 0, 9)
    mask = 9 | (8 << 8) | (7 << 16) | (6 << 24)
    ds2 = runtime.Dataset(ctx, 1, 5, 3)
    for flags in (0, _abi.IMAGE_WHITE_TRANSPARENT, _abi.IMAGE_BLACK_TRANSPARENT, _abi.IMAGE_WHITE_TRANSPARENT | _abi.IMAGE_BLACK_TRANSPARENT):
        ds2.set_image(0, small, flags=flags, mask_color=mask)
        got = ds2.get_image(0)
        want = ref.from_rgba8_64(small, bool(flags & 1), bool(flags & 2), mask)
        assert ref.half_steps(got, want).max() <= 1
        assert (got[1, 2] == -1).all() and (got[..., 3].view(np.uint16) == want[..., 3].view(np.uint16)).all()
        assert (got[0, 0] == 0).all() == bool(flags & 1) and (got[0, 1] == 0).all() == bool(flags & 2)
        assert got[2, 4, 3] > 0 and got[2, 3, 3] > 0   # almost white, almost black: untouched
    ds2.set_image(0, small, mask_color=0)
    assert (ds2.get_image(0)[1, 2] >= 0).all()
    ds.close(); ds2.close()


# ---- rays, small shapes -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_datasets(ctx):
    """per (n_images, resolution): cameras that move, with every rolling-shutter term, images of random halves -- built once"""
    sets = {}
    for n_images in (1, 3, 7):
        for (W, H) in ((5, 3), (64, 48)):
            cams = np.stack([orbit_record(25.0 + 40.0 * k, W, moving=True, pp=(0.47, 0.55), rs=(0.1, 0.3, -0.2, 0.25), focal_ratio=1.1) for k in range(n_images)])
            images = random_images(n_images, W, H, seed=n_images)
            sets[n_images, W] = (cams, images, make_dataset(ctx, cams, images))
    return sets


@pytest.mark.parametrize("n_images", [1, 3, 7])
@pytest.mark.parametrize("n_rays", [1, 63, 64, 65, 1000, 4096])
def test_rays_small_shapes(small_datasets, n_rays, n_images):
    """pixels, jitter, targets and backgrounds bit for bit; a second call bit-identical; the rays within 1e-5 of the float32 twin -- a few float32 steps of numbers no
    larger than 2 are 1e-6, a ray built from another image's camera is off by far more (the lens test judges them to the unit).  1000 rays over 7 images puts image
    boundaries inside waves: the branch that reads the camera per lane."""
    wrap = ((1 << 32) // n_images - max(n_rays // 2, 1)) & 0xffffffff   # (i + total) * n_images passes 2^32 inside the batch
    for (W, H) in ((5, 3), (64, 48)):
        cams, images, ds = small_datasets[n_images, W]
        for total in (0, 12345, wrap):
            for snap in (True, False):
                want = ref.rays32(SEED, cams, images, n_rays, total, snap)
                for random_bg in (True, False):
                    rays, jitter, target, background, pixels = gpu_rays(ds, n_rays, total, snap, random_bg)
                    where = (n_rays, n_images, W, total, snap, random_bg)
                    assert (pixels.view(np.uint32) == want["pixels"]).all(), where
                    assert same_bits(jitter, want["jitter"]) and same_bits(target, want["target"]), where
                    assert (background is None) == (not random_bg) and (background is None or same_bits(background, want["background"])), where
                    assert np.isfinite(rays).all() and np.abs(rays - want["rays"]).max() < 1e-5, where
                again = gpu_rays(ds, n_rays, total, snap, True)
                first = gpu_rays(ds, n_rays, total, snap, True)
                assert all(same_bits(a, b) for a, b in zip(again, first)), "two calls with the same inputs give the same bits"
    if n_images > 1 and n_rays >= 64:
        img = ref.rays32(SEED, cams, images, n_rays, 0, True)["pixels"][:, 0]
        assert len(set(img.tolist())) == n_images
        if (n_rays, n_images) == (1000, 7):
            waves = [set(img[k:k + 64].tolist()) for k in range(0, n_rays, 64)]
            assert any(len(w) > 1 for w in waves) and any(len(w) == 1 for w in waves), "both camera branches run"


# ---- rays, lenses -----------------------------------------------------------------------------------------------------------------------------------------------
LENSES = {0: (), 1: (0.0578421, -0.0805099, -0.000980296, 0.00015575), 2: (0.002, 0.0105, 1.0e-5, -2.0e-7, 1.0e-9, 64.0, 48.0)}


def ray_errors(got, want64):
    """(worst origin error relative to the origin's norm, worst direction error, worst | |d| - 1 |), in units of 2^-23"""
    o, d = got[:, :3].astype(np.float64), got[:, 3:].astype(np.float64)
    eo = np.abs(o - want64[:, :3]).max(1) / np.linalg.norm(want64[:, :3], axis=1)
    ed = np.abs(d - want64[:, 3:]).max(1)
    return eo.max() / UNIT, ed.max() / UNIT, np.abs(np.linalg.norm(d, axis=1) - 1.0).max() / UNIT


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_rays_lenses(ctx, mode):
    W, H, n_images, n_rays = 64, 48, 3, 1000
    cams = np.stack([orbit_record(10.0 + 50.0 * k, W, mode, LENSES[mode], moving=True, pp=(0.46, 0.53), rs=(0.15, 0.25, -0.3, 0.4), focal_ratio=1.13) for k in range(n_images)])
    images = random_images(n_images, W, H)
    ds = make_dataset(ctx, cams, images)
    for snap in (True, False):
        want32, want64 = ref.rays32(SEED, cams, images, n_rays, 777, snap), ref.rays64(SEED, cams, images, n_rays, 777, snap)
        rays = gpu_rays(ds, n_rays, 777, snap)[0]
        assert np.isfinite(rays).all() and np.isfinite(want64["rays"]).all()
        twin = ray_errors(want32["rays"].astype(np.float32), want64["rays"])
        gpu = ray_errors(rays, want64["rays"])
        print(f"mode {mode} snap {snap}: error in units of 2^-23 (origin, direction, |d| - 1): GPU {gpu[0]:.2f} {gpu[1]:.2f} {gpu[2]:.2f}; "
              f"float32 twin {twin[0]:.2f} {twin[1]:.2f} {twin[2]:.2f} over {n_rays} rays (none left out)")
        assert gpu[0] <= 4 * twin[0] and gpu[1] <= 4 * twin[1]
        assert gpu[2] <= 4 * twin[1], "|d| = 1 to the same unit"
    ds.close()


def test_f_theta_centre_pixel(ctx):
    """norm == 0: odd resolution, principal point 0.5, snap on, a draw in the centre pixel -- exactly the rotated (0, 0, 1)"""
    W, H, n_rays = 5, 3, 1000
    cams = np.stack([orbit_record(70.0, W, 2, (0.0, 0.2, 0.0, 0.0, 0.0, 5.0, 3.0))])
    images = random_images(1, W, H)
    ds = make_dataset(ctx, cams, images)
    rays, _, _, _, pixels = gpu_rays(ds, n_rays, 0, True)
    centre = pixels[:, 1] == 2 + 1 * W
    assert 20 < centre.sum() < n_rays
    col2 = cams[0][6:9]
    z = (np.float32(0) * cams[0][0:3] + (np.float32(0) * cams[0][3:6] + col2)).astype(np.float32)
    want = z / np.sqrt(z[0] * z[0] + (z[1] * z[1] + z[2] * z[2]), dtype=np.float32)
    assert all(same_bits(r[3:], want) for r in rays[centre])
    assert same_bits(rays[centre], ref.rays32(SEED, cams, images, n_rays, 0, True)["rays"][centre])
    assert not any(same_bits(r[3:], want) for r in rays[~centre][:50])
    ds.close()


# ---- masked pixels, and the hand-over to the sample generator -----------------------------------------------------------------------------------------------------
def test_masked_pixels(ctx, full_network):
    from nerfshop_amd import runtime
    W, H, n_rays = 16, 12, 1000
    img = np.random.default_rng(4).integers(1, 256, (2, H, W, 4), dtype=np.uint8)
    mask = 0x04030201
    img[:, :, 5] = (1, 2, 3, 4)
    ds = runtime.Dataset(ctx, 2, W, H)
    cams = [orbit_record(30.0 + 90.0 * k, W) for k in range(2)]
    for k in range(2):
        ds.set_image(k, img[k], mask_color=mask)
        ds.set_camera(k, ref.to_struct(cams[k]))
    assert (ds.get_image(0)[:, 5] == -1).all() and (ds.get_image(1)[:, 4] >= 0).all()
    out = ds.rays(n_rays, 0, ref.rng_of(SEED))
    rays, _, target, _, pixels = [t.cpu().numpy() for t in out]
    dead = pixels[:, 1] % W == 5
    assert 20 < dead.sum() < n_rays // 4
    assert (rays[dead, 3:] == 0).all() and (target[dead] == 0).all() and np.isfinite(rays).all()
    assert np.allclose(np.linalg.norm(rays[~dead, 3:], axis=1), 1.0, atol=1e-6)
    for k in range(2):
        assert (rays[dead & (pixels[:, 0] == k), :3] == cams[k][9:12]).all(), "a dead ray starts at its camera"
    coords, numsteps, ray_indices, counters = full_network.training_samples(None, out[0], out[1], 0.0, 1 << 20)   # (room for 1000 rays of 1024 samples: none is dropped)
    torch.cuda.synchronize()
    emitted = int(counters[0])
    idx = ray_indices.cpu().numpy()[:emitted]
    assert not dead[idx].any(), "no dead ray is emitted"
    assert int((~dead).sum()) >= emitted > 0.5 * int((~dead).sum()), "most live rays of these cameras cross the box"
    ds.close()


def test_through_the_generator(ctx, full_network):
    """dataset.rays -> training_samples against the twin's rays and jitter (uploaded) -> training_samples: the outputs are in the layout the next stage reads.  Rays
    whose bits equal the twin's must get the same samples; if every ray does, everything is compared bit for bit."""
    W, H, n_rays = 64, 48, 1000
    cams = np.stack([orbit_record(20.0 + 60.0 * k, W, pp=(0.48, 0.52)) for k in range(3)])
    images = random_images(3, W, H)
    ds = make_dataset(ctx, cams, images)
    want = ref.rays32(SEED, cams, images, n_rays, 4096, True)
    out = ds.rays(n_rays, 4096, ref.rng_of(SEED))
    a = full_network.training_samples(None, out[0], out[1], 0.0, 1 << 20)
    b = full_network.training_samples(None, torch.from_numpy(want["rays"]).to(DEV), torch.from_numpy(want["jitter"]).to(DEV), 0.0, 1 << 20)
    torch.cuda.synchronize()
    rays = out[0].cpu().numpy()
    equal = (rays.view(np.uint32) == want["rays"].view(np.uint32)).all(1)
    print(f"through the generator: {int(equal.sum())} of {n_rays} rays equal the float32 twin's in every bit")
    assert equal.mean() > 0.5

    def counts(r):
        n = int(r[3][0])
        c = np.zeros(n_rays, np.int64)
        c[r[2].cpu().numpy()[:n]] = r[1].cpu().numpy()[:n, 0]
        return c
    ca, cb = counts(a), counts(b)
    assert ca.sum() > 10 * n_rays and (ca[equal] == cb[equal]).all()
    if equal.all():
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    ds.close()


# ---- mark_untrained -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aabb_scale", [1, 4])
def test_mark_untrained(ctx, aabb_scale):
    from nerfshop_amd import runtime, synth
    net = runtime.NerfNetwork(ctx, synth.model_desc(aabb_scale, log2_hashmap_size=14), cell_cache_bytes=0)
    cams = ref.corner_cameras(aabb_scale)
    W, H = 48, 32
    ds = make_dataset(ctx, cams, random_images(2, W, H))
    grid0 = ref.marked_grid(aabb_scale)   # positive and negative cells, seen and unseen
    for clear in (True, False):
        net.set_density_grid(grid0)
        ds.mark_untrained(net, clear_visible=clear)
        got = net.get_density_grid()
        want, near, seen = ref.mark_untrained_ref(grid0, cams, W, H, clear)
        assert near.mean() <= 0.001
        wrong = (got.view(np.uint32) != want.view(np.uint32)) & ~near
        print(f"aabb_scale {aabb_scale} clear {clear}: {int(wrong.sum())} cells differ outside the {int(near.sum())} within 1e-6 of the boundary; untrained {100 * (~seen).mean():.1f} %")
        assert not wrong.any()
        assert ((got == -1) | (got == 0) | (got == grid0)).all()
        bits = np.unpackbits(net.get_density_bitfield(), bitorder="little")
        assert (bits.sum() > 0) == (not clear)
        assert not bits[got < 0].any(), "no bit in an untrained cell"
        assert (net.get_density_bitfield() == synth.grid_to_bitfield(got)).all(), "rebuilt as set_density_grid rebuilds it"
    # an f-theta camera sees everything: nothing is marked
    ds.set_camera(1, ref.to_struct(ref.camera_record(np.eye(4)[:3], focal=(50.0, 50.0), mode=2, params=(0.0, 0.01, 0.0, 0.0, 0.0, 48.0, 32.0))))
    net.set_density_grid(np.abs(grid0))
    ds.mark_untrained(net, clear_visible=False)
    assert (net.get_density_grid() == np.abs(grid0)).all()
    ds.mark_untrained(net, clear_visible=True)
    assert (net.get_density_grid() == 0).all()
    ds.close(); net.close()


# ---- refusals and states --------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_states(ctx, full_network):
    from nerfshop_amd import _abi, runtime
    from nerfshop_amd._abi import NrsError
    import ctypes as C
    with pytest.raises(NrsError, match="n_images"):
        runtime.Dataset(ctx, 0, 4, 4)
    with pytest.raises(NrsError, match="width or height"):
        runtime.Dataset(ctx, 1, 4, 0)
    ds = runtime.Dataset(ctx, 2, 4, 3)
    img, cam = random_images(1, 4, 3)[0], ref.to_struct(orbit_record(10.0, 4))
    with pytest.raises(NrsError, match="index"):
        ds.set_image(2, img)
    with pytest.raises(NrsError, match="index"):
        ds.set_camera(2, cam)
    with pytest.raises(NrsError):
        ds.set_image(0, img[:2])   # the wrong shape never reaches the library
    with pytest.raises(NrsError, match="error -5.*never been set"):
        ds.get_image(0)
    ds.set_image(0, img)
    ds.set_camera(0, cam)
    ds.set_camera(1, cam)
    rng = ref.rng_of(SEED)
    with pytest.raises(NrsError, match="error -5.*image has never been set"):
        ds.rays(8, 0, rng)
    with pytest.raises(NrsError, match="error -5.*image has never been set"):
        ds.mark_untrained(full_network)
    ds.set_image(1, img)
    ds2 = runtime.Dataset(ctx, 1, 4, 3)
    ds2.set_image(0, img)
    with pytest.raises(NrsError, match="error -5.*camera has never been set"):
        ds2.rays(8, 0, rng)
    with pytest.raises(NrsError, match="error -5.*camera has never been set"):
        ds2.mark_untrained(full_network)
    with pytest.raises(NrsError, match="2\\^21"):
        ds.rays((1 << 21) + 1, 0, rng)
    out = ds.rays(0, 0, rng)
    assert out[0].shape == (0, 6) and out[4].shape == (0, 2)
    bad = _abi.TrainingCamera()
    bad.struct_size = 100
    with pytest.raises(NrsError, match="struct_size"):
        ds.set_camera(0, bad)
    p = _abi.DatasetRaysParams()
    p.struct_size = 0
    q = torch.zeros(64, device=DEV).data_ptr()
    assert ctx.lib.nrs_dataset_rays(ds.h, None, C.byref(p), 1, q, q, q, q, q) == -1
    other = runtime.Context(0)
    try:
        with pytest.raises(NrsError, match="different contexts"):
            runtime.Dataset(other, 1, 4, 3).mark_untrained(full_network)
    finally:
        other.close()
    # destroyed while nothing is in flight; a closed dataset is closed once
    ds.rays(64, 0, rng)
    torch.cuda.synchronize()
    ds.close(); ds.close(); ds2.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_fit_end_to_end(ctx, desc14):
    """A teacher rendered by this library from 8 orbit views at 32 x 32 (premultiplied linear RGBA, fed in as float32), a ninth view held out; Trainer.fit for 64 steps
    of 1024 rays.  The loss falls (test_trainer's criterion), the held-out view rendered from the EMA weights is closer to the teacher's than from the initial
    weights, and step_dataset returns while the device is still busy."""
    from nerfshop_amd import _abi, runtime, synth
    from nerfshop_amd.trainer import Trainer
    W = H = 32
    grid = synth.density_grid(1)
    tb = runtime.Testbed(ctx, desc14, 1)
    tb.nerf_network.set_params(synth.make_params(desc14))
    tb.nerf_network.set_density_grid(grid)
    buf = runtime.RenderBuffer(W, H)

    def render(network, camera):
        p = synth.render_params(W, H, camera)
        p.linear_colors = 1
        buf.clear_frame()
        tb.render_with_params(network, p, buf.frame_buffer(), buf.depth_buffer())
        torch.cuda.synchronize()
        return buf.frame_buffer().clone()

    azimuths = [45.0 * k for k in range(8)]
    ds = runtime.Dataset(ctx, 8, W, H)
    for k, az in enumerate(azimuths):
        frame = render(tb.nerf_network, synth.orbit_camera(az))
        assert float(frame[..., 3].max()) > 0.5, "the teacher's view shows the scene"
        ds.set_image(k, frame.contiguous())
        cam = _abi.TrainingCamera()
        cam.xform_start[:] = cam.xform_end[:] = synth.orbit_camera(az).tolist()
        focal = 0.5 * W / math.tan(0.5 * synth.CAMERA_ANGLE_X)
        cam.focal_length[:], cam.principal_point[:] = (focal, focal), (0.5, 0.5)
        ds.set_camera(k, cam)
    held_out = synth.orbit_camera(22.5, 35.0)
    truth = render(tb.nerf_network, held_out)

    trainer = Trainer(ctx, desc14, seed=11, max_samples=1 << 17)
    student = runtime.NerfNetwork(ctx, desc14, cell_cache_bytes=0)
    student.set_density_grid(grid)

    def held_out_error():
        student.set_params_device(trainer.optimizer.export_fp16(_abi.OPT_EXPORT_EMA))
        return float(((render(student, held_out) - truth) ** 2).mean())

    before = held_out_error()
    losses = trainer.fit(ds, 64, n_rays=1024)
    torch.cuda.synchronize()
    assert trainer.training_step == 64 and trainer.optimizer.step_count() == 64 and trainer.n_rays_total == 64 * 1024
    losses = [float(v) for v in losses]
    after = held_out_error()
    print("fit losses:", " ".join(f"{v:.5f}" for v in losses[:8]), "...", " ".join(f"{v:.5f}" for v in losses[-8:]))
    print(f"held-out view, mean squared error against the teacher: {before:.6f} before, {after:.6f} after")
    assert len(losses) == 64 and all(np.isfinite(losses)) and losses[0] > 0
    assert np.mean(losses[-8:]) < np.mean(losses[:8])
    assert after < before
    assert (trainer.network.get_density_grid() < 0).any(), "cells no camera sees stay untrained through the grid updates"
    # every buffer exists by now: a step allocates nothing, and returns with the stream still busy
    busy = torch.randn(8192, 8192, device=DEV)
    stream = torch.cuda.current_stream()
    torch.cuda.synchronize()
    for _ in range(6):
        busy = (busy @ busy) * 1e-4   # some tens of milliseconds of work ahead of the step
    trainer.step_dataset(ds, 1024)
    assert not stream.query(), "Trainer.step_dataset returned with the stream drained: it has waited for the device"
    torch.cuda.synchronize()
    ds.close()
