"""The training-ray path without a GPU: the twins of tests/ray_loss_ref.py are checked against each other and against hand-written numbers, the library's new
surface exists and refuses bad arguments before it touches a device, and the generator's twin is stable against the last bit of a ray's entry distance.

Which of these guard the library: test_surface_exists, test_struct_size_matches_the_library and test_bad_arguments_are_refused_without_a_device fail without the
feature.  The others (autograd against closed form, the hand-computed ray, the accuracy unit, the generator's stability) pin the TWIN that the GPU tests compare
the library with, not the library: they pass on any tree that holds tests/ray_loss_ref.py.  So do the tests of the large-scene inputs: the default batches are bit for bit what they
were before random_batch took dt_steps and aabb, the two big-box batches meet the conditions the GPU comparison needs, and the generator's four large-box cases
reach every cascade, the 1024-sample limit and an entry distance of 0."""
import ctypes as C

import numpy as np
import pytest
import torch

import ray_loss_ref as ref

COLOUR_PATHS = ((ref.LINEAR, False), (ref.SRGB, False), (ref.SRGB, True))


@pytest.mark.parametrize("loss_type", range(7))
@pytest.mark.parametrize("colour", COLOUR_PATHS)
def test_autograd_against_closed_form(loss_type, colour):
    """The restated formula ("T after the sample", suffix = C - C2, the additive terms) is the derivative autograd finds.  1e-9 relative to the size of the terms that
    form an element (the A of the accuracy unit: T rgb and the suffix cancel, so an element can be far smaller than its terms).  sigma dt stays below 5 per sample: past
    that the reference's own 1 - alpha loses digits even in float64.  Early stops are masked out of the loss by both; rays within 1e-6 of a kink are left out."""
    b = ref.random_batch(100 + loss_type, n_rays=60, max_count=70, ld=8, density_mean=4.5, density_max=6.5, loss_type=loss_type, color_space=colour[0], lin=colour[1],
                         l1=True, near_distance=0.6, with_origins=True, rgb_act_kind=ref.ACT_EXPONENTIAL if loss_type % 2 else ref.ACT_LOGISTIC)
    a, c = ref.composite_loss(b), ref.closed_form(b)
    assert int((c.f.M < c.f.N).sum()) >= 5, "the batch must hold early stops"
    assert torch.equal(a.numsteps_out, c.numsteps_out) and a.counter == c.counter
    kink = (ref.kink_distance(loss_type, c.f.target, c.f.C).min(1).values < 1e-6).numpy()
    used = (c.src >= 0).numpy()
    used[used] &= ~kink[c.ray_of.numpy()[used]]
    assert used.sum() > 500
    diff = (a.dl - c.dl).abs().numpy()[used]
    A = c.A.numpy()[used]
    worst = float((diff / np.maximum(A, 1e-300)).max())
    print(f"loss {loss_type} colour {colour}: autograd against closed form, worst |difference| / A = {worst:.3e} over {int(used.sum())} samples")
    assert (diff <= 1e-9 * A).all()
    assert float((a.loss - c.loss).abs().max()) == 0.0


def test_hand_computed_two_sample_ray():
    """L2, Logistic colours, Exponential density, one ray of two samples with sigma dt = 2.7295 and 1.0041, opaque target, black background, loss scale 128."""
    coords = np.zeros((2, 7), np.float32)
    coords[:, 3] = np.float32(0.2)  # dt = 0.2 * (16 - 1) * sqrt(3) / 1024 + sqrt(3) / 1024 = 0.0067658...
    b = dict(out=np.array([[0.0, 1.0, -1.0, 6.0], [2.0, 0.0, -2.0, 5.0]]), coords=coords, numsteps=np.array([[2, 0]]), target=np.array([[0.25, 0.5, 0.75, 1.0]], np.float32),
             background=None, origins=None, rgb_act=ref.ACT_LOGISTIC, den_act=ref.ACT_EXPONENTIAL, aabb=ref.AABB_UNIT,
             p=dict(loss_type=ref.L2, color_space=ref.LINEAR, lin=True, loss_scale=128.0, background=(0.0, 0.0, 0.0), near_distance=0.0, l1=False, cap=4))
    want_dl = np.array([[15.182823557510343, 9.599268908129986, -23.226809647952344, -1.1723414537504357],
                        [0.28203505256533373, 0.5398785562149123, -0.5486182349412776, 1.6389096574386999],
                        [0, 0, 0, 0], [0, 0, 0, 0]])
    for r in (ref.closed_form(b), ref.composite_loss(b)):
        assert r.numsteps_out.tolist() == [[2, 0]] and r.counter == 2
        np.testing.assert_allclose(r.f.C.detach().numpy()[0], [0.503791535433204, 0.7040294605151838, 0.25632142017117765], rtol=1e-12)
        np.testing.assert_allclose(float(r.f.T.detach()[0]), 0.023905055920289714, rtol=1e-12)  # (1 - 0.93474992) (1 - 0.63363942)
        np.testing.assert_allclose(float(r.loss[0]), 0.1165855681324877, rtol=1e-12)
        np.testing.assert_allclose(r.dl.numpy(), want_dl, rtol=1e-10, atol=0)
    r32 = ref.closed_form32(b)
    np.testing.assert_allclose(r32.dl.numpy(), want_dl, rtol=2e-5)


def test_surface_exists(built):
    from nerfshop_amd import _abi, runtime, torch_module
    lib = _abi.load()
    for name in ("nrs_training_samples", "nrs_ray_loss"):
        assert hasattr(lib, name) and name in _abi.EXPORTS
    assert lib.nrs_abi_version() == 3
    assert callable(getattr(runtime.NerfNetwork, "ray_loss", None)) and callable(getattr(runtime.Testbed, "training_samples", None))
    assert callable(torch_module.ray_loss) and callable(getattr(torch_module.NerfNetworkModule, "ray_step", None))
    p = _abi.RayLossParams(max_samples_compacted=5)
    assert (p.loss_type, p.loss_scale, p.color_space, p.train_in_linear_colors, p.max_samples_compacted) == (_abi.LOSS_L2, 128.0, _abi.COLOR_LINEAR, 0, 5)
    assert p.struct_size == C.sizeof(_abi.RayLossParams) == 44
    assert [_abi.LOSS_L2, _abi.LOSS_L1, _abi.LOSS_MAPE, _abi.LOSS_SMAPE, _abi.LOSS_HUBER, _abi.LOSS_LOG_L1, _abi.LOSS_RELATIVE_L2] == list(range(7))


def _ray_loss_call(lib, model, params, **over):
    buf = np.zeros(64, np.float32)
    q = buf.ctypes.data
    a = dict(model=model, stream=None, params=params, n_rays=1, counter=None, numsteps=q, n_samples=1, coords=q, ld_in=7, output=q, ld_out=1, out_layout=0, target=q,
             background=None, origins=None, numsteps_out=q + 64, coords_out=q, dl=q, ld_dl=8, dl_layout=0, loss=None, counter_out=q)
    a.update(over)
    status = lib.nrs_ray_loss(*a.values())
    return status, lib.nrs_last_error()


def test_struct_size_matches_the_library(built):
    """A struct of the mirror's size passes the size check (and is then refused for its loss type); any other size is refused for its size."""
    from nerfshop_amd import _abi
    lib = _abi.load()
    fake = C.c_void_p(np.zeros(64, np.float32).ctypes.data)  # never dereferenced before the argument checks
    p = _abi.RayLossParams(max_samples_compacted=4, loss_type=99)
    status, msg = _ray_loss_call(lib, fake, C.byref(p))
    assert status == -1 and b"loss_type" in msg
    for wrong in (0, 40, 48):
        p.struct_size = wrong
        status, msg = _ray_loss_call(lib, fake, C.byref(p))
        assert status == -1 and b"struct_size" in msg


def test_bad_arguments_are_refused_without_a_device(built):
    from nerfshop_amd import _abi
    lib = _abi.load()
    INVALID = -1
    keep = np.zeros(64, np.float32)
    fake = C.c_void_p(keep.ctypes.data)
    good = _abi.RayLossParams(max_samples_compacted=4)
    assert _ray_loss_call(lib, None, C.byref(good))[0] == INVALID
    assert b"NULL" in lib.nrs_last_error()
    for name in ("params", "numsteps", "coords", "output", "target", "numsteps_out", "coords_out", "dl", "counter_out"):
        over = {name: None}
        status, msg = _ray_loss_call(lib, fake, over.pop("params", C.byref(good)), **over)
        assert status == INVALID and b"NULL" in msg, name
    q = keep.ctypes.data
    for over, word in ((dict(numsteps=q, numsteps_out=q), b"aliases"), (dict(ld_in=6), b"ld_in"), (dict(out_layout=2), b"layout"), (dict(dl_layout=7), b"layout"),
                       (dict(n_samples=9, ld_out=8), b"ld_out"), (dict(ld_dl=3), b"ld_dl"), (dict(), b"overlaps")):  # (the helper's coords_out is its coords)
        status, msg = _ray_loss_call(lib, fake, C.byref(good), **over)
        assert status == INVALID and word in msg, over
    for field, value, word in (("color_space", 2, b"color_space"), ("max_samples_compacted", 0, b"max_samples_compacted"), ("near_distance", 0.5, b"d_ray_origins"),
                               ("loss_scale", float("inf"), b"loss_scale")):
        p = _abi.RayLossParams(**{"max_samples_compacted": 4, field: value})
        status, msg = _ray_loss_call(lib, fake, C.byref(p))
        assert status == INVALID and word in msg, field
    # the generator: NULLs, ld < 7, max_samples == 0
    ts = lib.nrs_training_samples
    assert ts(None, None, 1, q, None, 0.0, 8, q, 7, q, q, q) == INVALID
    for k in (3, 7, 9, 10, 11):
        args = [fake, None, 1, q, None, 0.0, 8, q, 7, q, q, q]
        args[k] = None
        assert ts(*args) == INVALID and b"NULL" in lib.nrs_last_error(), k
    assert ts(fake, None, 1, q, None, 0.0, 8, q, 6, q, q, q) == INVALID and b"ld < 7" in lib.nrs_last_error()
    assert ts(fake, None, 1, q, None, 0.0, 0, q, 7, q, q, q) == INVALID and b"max_samples" in lib.nrs_last_error()
    assert ts(fake, None, 1, q, None, -1.0, 8, q, 7, q, q, q) == INVALID and b"cone_angle_constant" in lib.nrs_last_error()


def test_the_accuracy_unit():
    """The reference's own float32 gap: closed_form32, stored as fp16 like the kernel's result, against closed_form in the units every GPU comparison uses (printed;
    the GPU's bar is four times this figure on the same inputs)."""
    for name, b in (("constructed", ref.constructed_batch(3)[0]), ("random L2", ref.random_batch(140)), ("random Huber sRGB", ref.random_batch(144, loss_type=ref.HUBER, color_space=ref.SRGB))):
        c, c32 = ref.closed_form(b), ref.closed_form32(b)
        same = (c32.f.M == c.f.M).numpy() & ~c.f.near_threshold.numpy()
        used = (c.src >= 0).numpy()
        used[used] &= same[c.ray_of.numpy()[used]]
        err = ref.error_units(ref.to_fp16_values(c32.dl.numpy()[used]), c.dl.numpy()[used], c.A.numpy()[used])
        print(f"{name}: closed_form32 against closed_form, worst error per row {err.max(0)} units of 2^-23 A over {int(used.sum())} samples")
        assert np.isfinite(err).all()


def _batch_hash(b):
    import hashlib
    m = hashlib.sha256()
    for k in ("out", "coords", "numsteps", "target", "background", "origins"):
        m.update(k.encode())
        m.update(b"none" if b[k] is None else np.ascontiguousarray(b[k]).tobytes())
    m.update(repr((b["rgb_act"], b["den_act"], b["aabb"], sorted(b["p"].items()))).encode())
    return m.hexdigest()


def test_default_batches_are_what_they_were():
    """random_batch and constructed_batch took dt_steps and aabb after these hashes were taken (of test_activations' batch 74, test_every_loss_and_colour_path's
    batch 140 and the constructed batch): their defaults give the same bytes."""
    assert _batch_hash(ref.random_batch(74, rgb_act_kind=1, den_act_kind=0, l1=True, near_distance=0.7, with_origins=True, loss_type=ref.HUBER)) == \
        "8d36b56a06d18f057850bef3b4d3353a3c6b3b6c02a2168b85a2c6e77e434eb4"
    assert _batch_hash(ref.random_batch(140)) == "b0a095b130f5136bb0ee32caa994f98f833f84ae9b4bfcfaa4ab766745afa928"
    assert _batch_hash(ref.constructed_batch(3)[0]) == "f19bea9e51c71d06f1803d5edf313c3e1149da5e502dd8c370a234674feaa3d5"


@pytest.mark.parametrize("scale", [16, 4])
def test_big_box_batches_are_what_the_gpu_tests_need(scale):
    """The two batches of tests/test_gpu_ray_loss.py::test_long_steps_in_a_big_box, judged with the twins alone: conditions on the INPUTS, so that the GPU comparison
    covers what it is for -- steps up to 128 minimum steps (warped dt up to 8.47), rays that stop early and rays that do not, samples on both sides of the near
    distance and none so close to it that float32 could not decide, the float32 twin consuming what the float64 twin consumes, and gradients that an fp16 holds."""
    b = ref.big_box_batch(scale)
    assert b["aabb"] == ref.scene_aabb(scale) and b["p"]["near_distance"] == {16: 6.0, 4: 1.5}[scale]
    c, c32 = ref.closed_form(b), ref.closed_form32(b)
    f = c.f
    wdt = b["coords"][:, 3]
    assert wdt.max() > 8.0 and wdt.min() < 0.1
    left_out = float(f.near_threshold.numpy().mean())
    has = (f.N > 0).numpy()
    stopped = float(((f.M < f.N).numpy() & has).sum() / has.sum())
    used = (c.src >= 0).numpy()
    src, ray_of = c.src.numpy()[used], c.ray_of.numpy()[used]
    mn, mx = (np.asarray(v, np.float64) for v in b["aabb"])
    dist = np.linalg.norm(mn + b["coords"][src, :3].astype(np.float64) * (mx - mn) - b["origins"][ray_of].astype(np.float64), axis=1)
    near = float(np.float32(b["p"]["near_distance"]))
    within, closest = float((dist < near).mean()), float(np.abs(dist / near - 1.0).min())
    normal = float((np.abs(c.dl.numpy()[used]) >= 2.0 ** -14).mean())
    print(f"big box, scale {scale}: left out {left_out:.3f}, stopped early {stopped:.3f}, within the near distance {within:.3f} (closest {closest:.1e} relative), "
          f"fp16-normal {normal:.3f}, warped dt max {wdt.max():.2f}, raw density min {b['out'][:, 3].min():.2f}")
    assert left_out <= 0.01
    assert 0.1 <= stopped <= 0.6
    assert 0.05 <= within <= 0.5
    assert closest > 1e-6
    assert torch.equal(c32.f.M, f.M)
    assert normal >= 0.3


def test_large_scene_rays_cover_what_they_are_for(built):
    """The generator's four large-box cases (tests/test_gpu_training_large_scenes.py) through the twin alone: every cascade the cone reaches, steps beyond 16
    minimum steps, a ray on the 1024-sample limit, cameras inside the box, stable counts."""
    from oracle import oracle as orc
    lib = orc.load()
    walks = {case: ref.large_scene_walk(lib, *case) for case in ref.LARGE_SCENE_CASES}
    for (scale, cone), w in walks.items():
        print(f"scale {scale} cone {cone:.5f}: {len(w.rays)} rays, {int((w.counts > 0).sum())} with samples, {int(w.counts.sum())} samples, per cascade {w.per_cascade.tolist()}, "
              f"stable {w.stable.mean():.3f}, entry distance 0: {int((w.tmin == 0).sum())}, on the limit {int((w.counts == 1024).sum())}, warped dt max {w.max_warped_dt:.2f}")
    ref.assert_large_scene_coverage(walks)


@pytest.fixture(scope="module")
def outside_rays(built):
    """100 unit rays from origins outside the unit box towards points inside it, and a jitter per ray"""
    rng = np.random.default_rng(21)
    o = rng.normal(size=(100, 3))
    o = (0.5 + 1.6 * o / np.linalg.norm(o, axis=1, keepdims=True)).astype(np.float32)
    d = rng.uniform(0.3, 0.7, (100, 3)).astype(np.float32) - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return np.concatenate([o, d], 1).astype(np.float32), rng.random(100).astype(np.float32)


def test_generator_twin_is_stable_against_the_entry_distance(scene, outside_rays):
    """A ray whose sample count changes when its entry distance moves by two float32 steps cannot be compared bit for bit across two implementations of the box
    intersection; the GPU test leaves such rays out, and this keeps their share below 2 % for the twin alone."""
    from oracle import oracle as orc
    lib = orc.load()
    rays, jitter = outside_rays
    counts = [np.array([len(r) for r in ref.march(lib, scene.bitfield, ref.AABB_UNIT, rays, jitter, 0.0, tmin_nudge_ulps=k)]) for k in (-2, 0, 2)]
    stable = (counts[0] == counts[1]) & (counts[1] == counts[2])
    print(f"stable rays: {int(stable.sum())} of {len(stable)}; rays with samples: {int((counts[1] > 0).sum())}, samples {int(counts[1].sum())}")
    assert (counts[1] > 0).sum() >= 30
    assert stable.mean() >= 0.98
