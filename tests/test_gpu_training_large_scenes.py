"""The training path where real captures live: boxes of side 4 and 16 (aabb_scale > 1), cone steps (cone_angle_constant 1 / 256), cascades above 0 and cameras
that stand inside the box.  The other GPU tests of that path (tests/test_gpu_ray_loss.py, test_gpu_optimizer.py::test_trainer, test_gpu_dataset.py::
test_fit_end_to_end) run in the unit box with a constant step on rays that start outside it.

A. nrs_training_samples against the twin's walk (ray_loss_ref.march, on the oracle's scalars) in four cases, aabb_scale {4, 16} x cone {0, 1 / 256}, through an
   occupancy in which every 4 x 4 x 4 block of every cascade is occupied with probability 0.3, on ray_loss_ref.large_scene_rays: from outside the box, from inside it,
   from inside the unit cube, axis-parallel, missing, starting on a face.  Counts and records of every stable ray equal the twin's bit for bit.  What the cases must
   exercise (every cascade the cone reaches, warped dt above 1, the 1024-sample limit, entry distance 0) is asserted from the twin, here and in
   tests/test_ray_loss_host.py.
C. Trainer.step's gather of per-ray inputs by the generator's ray slots, with rays that miss the box inside the batch; and Trainer.fit end to end at aabb_scale 4
   with max_cascade 2 and the cone on.
(B, the ray loss at long steps in a big box, is in tests/test_gpu_ray_loss.py.)  The measured figures are in profiles/training_large_scenes.md."""
import math

import numpy as np
import pytest
import torch

import ray_loss_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CONE = 1.0 / 256.0


@pytest.fixture(scope="module")
def ctx(built):
    from nerfshop_amd import runtime
    return runtime.Context(0)


# ---- A: the generator ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def walks(built):
    """the twin's walk of the four cases, once"""
    from oracle import oracle as orc
    lib = orc.load()
    return {case: ref.large_scene_walk(lib, *case) for case in ref.LARGE_SCENE_CASES}


@pytest.fixture(scope="module")
def networks(ctx, walks):
    """per aabb_scale a model of that box that holds the case's occupancy"""
    from nerfshop_amd import runtime, synth
    nets = {}
    for (scale, cone), w in walks.items():
        if scale not in nets:
            nets[scale] = runtime.NerfNetwork(ctx, synth.model_desc(scale, log2_hashmap_size=14), cell_cache_bytes=0)
            nets[scale].set_density_bitfield(w.bitfield)
    return nets


def counts_of(n_rays, numsteps, ray_indices, counters):
    emitted = int(counters[0])
    got = np.zeros(n_rays, np.int64)
    got[ray_indices[:emitted]] = numsteps[:emitted, 0]
    return got


def test_the_cases_cover_what_they_are_for(walks):
    ref.assert_large_scene_coverage(walks)


@pytest.mark.parametrize("scale,cone", ref.LARGE_SCENE_CASES)
def test_training_samples_against_the_twin_in_large_boxes(walks, networks, scale, cone):
    w, net = walks[scale, cone], networks[scale]
    n = len(w.rays)
    total = int(w.counts.sum())
    max_samples = total + 2048 + 11   # (room for an unstable ray's other count: the layout below is judged on the counts the generator gave)
    d_rays, d_jitter = torch.from_numpy(w.rays).to(DEV), torch.from_numpy(w.jitter).to(DEV)
    runs = [[x.cpu().numpy() for x in net.training_samples(None, d_rays, d_jitter, cone, max_samples, ld=8)] for _ in range(2)]
    for x, y in zip(*runs):
        assert x.tobytes() == y.tobytes(), "two calls agree byte for byte"
    coords, numsteps, ray_indices, counters = runs[0]
    emitted = int(counters[0])
    got_counts = counts_of(n, numsteps, ray_indices, counters)
    print(f"scale {scale} cone {cone:.5f}: {n} rays, {int((w.counts > 0).sum())} with samples, twin {total} samples, GPU {int(counters[1])}; per cascade "
          f"{w.per_cascade.tolist()}; stable {w.stable.mean():.3f}; rays whose count differs from the twin's: {int((got_counts != w.counts).sum())}")
    assert (got_counts[w.stable] == w.counts[w.stable]).all(), "stable rays have the twin's sample count"
    assert got_counts[w.missing] == 0, "the ray that misses the box has no samples"
    assert got_counts.max() <= 1024
    want_numsteps, want_idx, want_counters, bases = ref.layout_from_counts(got_counts, max_samples)
    assert emitted == want_counters[0] and int(counters[1]) == want_counters[1] <= max_samples
    assert (ray_indices[:emitted] == want_idx).all() and (numsteps[:emitted] == want_numsteps).all()
    assert (numsteps[emitted:] == 0).all() and (ray_indices[emitted:] == 0).all()
    compared = 0
    for i in np.nonzero(w.stable & (w.counts > 0))[0]:
        rec = coords[bases[i]:bases[i] + w.counts[i], :7]
        assert (rec.view(np.uint32) == w.walk[i].view(np.uint32)).all(), f"ray {i}: records differ from the twin's"
        compared += len(rec)
    assert compared >= 0.9 * total
    end = int(want_counters[1])
    assert (coords[end:, :7] == 0).all() and (coords[:, 7] == 0).all(), "zero tail; float 7 of a record is never written"


def test_testbed_cone_default_in_a_large_scene(ctx, walks):
    """A Testbed of aabb_scale 16 marches training rays with the cone of 1 / 256 when none is given."""
    from nerfshop_amd import runtime, synth
    w = walks[16, CONE]
    tb = runtime.Testbed(ctx, synth.model_desc(16, log2_hashmap_size=14), aabb_scale=16)
    assert tb.cone_angle_constant == CONE
    tb.nerf_network.set_density_bitfield(w.bitfield)
    d_rays, d_jitter = torch.from_numpy(w.rays).to(DEV), torch.from_numpy(w.jitter).to(DEV)
    implied = [x.cpu().numpy() for x in tb.training_samples(d_rays, d_jitter, 1 << 15)]
    stated = [x.cpu().numpy() for x in tb.training_samples(d_rays, d_jitter, 1 << 15, cone_angle_constant=CONE)]
    without = [x.cpu().numpy() for x in tb.training_samples(d_rays, d_jitter, 1 << 15, cone_angle_constant=0.0)]
    for x, y in zip(implied, stated):
        assert x.tobytes() == y.tobytes()
    assert int(implied[3][1]) == int(counts_of(len(w.rays), *implied[1:]).sum()) > 5000
    assert int(without[3][1]) > 2 * int(implied[3][1]), "a constant step takes several times the samples"
    tb.nerf_network.close()


def test_drops_in_a_large_scene(walks, networks):
    """test_training_samples_drops_clips_and_repeats' assertions at aabb_scale 16 with the cone on: max_samples cuts inside the batch."""
    w, net = walks[16, CONE], networks[16]
    d_rays, d_jitter = torch.from_numpy(w.rays).to(DEV), torch.from_numpy(w.jitter).to(DEV)
    full = [x.cpu().numpy() for x in net.training_samples(None, d_rays, d_jitter, CONE, 1 << 15)]
    got_counts = counts_of(len(w.rays), *full[1:])
    assert int(full[3][1]) == got_counts.sum() <= 1 << 15
    cut = int(got_counts.sum()) * 2 // 3
    runs = [[x.cpu().numpy() for x in net.training_samples(None, d_rays, d_jitter, CONE, cut)] for _ in range(2)]
    for x, y in zip(*runs):
        assert x.tobytes() == y.tobytes()
    coords, numsteps, ray_indices, counters = runs[0]
    want_numsteps, want_idx, want_counters, bases = ref.layout_from_counts(got_counts, cut)
    assert 0 < want_counters[0] < (got_counts > 0).sum()
    assert tuple(counters) == want_counters and (numsteps[:counters[0]] == want_numsteps).all() and (ray_indices[:counters[0]] == want_idx).all()
    dropped = np.nonzero(got_counts > 0)[0][want_counters[0]:]
    assert len(dropped) and not np.isin(dropped, ray_indices[:counters[0]]).any(), "the ray that does not fit and every later one are dropped"
    end = int(want_numsteps[-1].sum())
    assert (coords[:end] == full[0][:end]).all() and (coords[end:] == 0).all()


# ---- C: the Trainer -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def desc4():
    from nerfshop_amd import synth
    return synth.model_desc(4, log2_hashmap_size=14)


def test_step_gathers_by_ray_slot(ctx, desc4):
    """96 rays at aabb_scale 4 of which every third misses the box, so that the generator's ray slots are not the rays' indices; and the same rays with the missing
    ones moved to the end, where they are.  One Trainer.step on each from the same weights, seed and grid (max_cascade 2, cone 1 / 256): a ray's samples and its loss
    are functions of the ray alone and both batches share the normaliser, so the per-ray losses -- the step's loss buffer, mapped back through ray_indices -- are
    bit-identical.  A gather by anything but the slot's ray gives a ray another ray's target."""
    from nerfshop_amd import synth
    from nerfshop_amd.trainer import Trainer
    rng = np.random.default_rng(77)
    n = 96
    o = rng.uniform(0.5 - 0.45 * 4, 0.5 + 0.45 * 4, (n, 3))
    d = rng.uniform(0.0, 1.0, (n, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    miss = np.arange(n) % 3 == 2
    o[miss] = [0.5 - 3.0, 0.5, 0.5] + rng.uniform(-0.2, 0.2, (int(miss.sum()), 3))   # outside the box, looking away from it
    d[miss] = [-1.0, 0.0, 0.0]
    rays = np.concatenate([o, d], 1).astype(np.float32)
    a = rng.choice(np.array([0.0, 0.5, 1.0], np.float32), n)
    target = np.concatenate([rng.random((n, 3)).astype(np.float32) * a[:, None], a[:, None]], 1).astype(np.float32)
    jitter = rng.random(n).astype(np.float32)
    order = np.concatenate([np.nonzero(~miss)[0], np.nonzero(miss)[0]])
    grid = synth.density_grid(4)

    def one_step(idx):
        trainer = Trainer(ctx, desc4, seed=11, density_grid=grid, max_samples=1 << 16, max_cascade=2, cone_angle_constant=CONE)
        r, t, j = (torch.from_numpy(np.ascontiguousarray(x[idx])).to(DEV) for x in (rays, target, jitter))
        _, numsteps, ray_indices, counters = trainer.network.training_samples(None, r, j, CONE, 1 << 16)
        total = trainer.step(r, t, jitter=j)
        torch.cuda.synchronize()
        emitted = int(counters[0])
        assert int(counters[1]) <= 1 << 16, "no ray is dropped"
        slots = ray_indices.cpu().numpy()[:emitted]
        per_ray = np.zeros(n, np.float32)
        has = np.zeros(n, bool)
        per_ray[idx[slots]] = trainer._bufs.loss.cpu().numpy()[:emitted]
        has[idx[slots]] = True
        return per_ray, has, float(total), slots

    first, has_first, total_first, slots_first = one_step(np.arange(n))
    second, has_second, total_second, slots_second = one_step(order)
    assert not has_first[miss].any() and has_first.sum() >= 40, "the missing rays have no samples, most others do"
    assert (slots_first != np.arange(len(slots_first))).any(), "the first batch's slots are not the identity"
    assert (slots_second == np.arange(len(slots_second))).all(), "the second batch's are"
    assert (has_first == has_second).all()
    assert (first[has_first] > 0).all()
    assert first.tobytes() == second.tobytes(), "a ray's loss does not depend on where the ray stands in the batch"
    assert total_first > 0 and abs(total_first - total_second) <= 1e-6 * total_first
    assert abs(total_first - float(first.astype(np.float64).sum())) <= 1e-5 * total_first


def make_teacher4(ctx, desc4):
    """A teacher at aabb_scale 4 (the synthetic scene as conftest.Scene builds it), rendered from 8 views at 32 x 32 into a Dataset, and a ninth view held out.  Its
    frames are rendered with linear_colors: the synthetic network's colours are taken as they are, which makes the images linear premultiplied RGBA.  The
    cameras are synth's orbit at the scale conftest.Scene.camera gives a box of side 16 (0.33 x 6), in proportion to the box: inside it, outside the unit cube."""
    from nerfshop_amd import _abi, runtime, synth
    W = H = 32
    cam_scale = 0.33 * 6.0 * 4.0 / 16.0
    grid = synth.density_grid(4)
    tb = runtime.Testbed(ctx, desc4, 4)
    tb.nerf_network.set_params(synth.make_params(desc4, sigma_raw=synth.default_sigma_raw(4), aabb_scale=4))
    tb.nerf_network.set_density_grid(grid)
    buf = runtime.RenderBuffer(W, H)

    def render(network, camera, linear_colors=1):
        p = synth.render_params(W, H, camera, aabb_scale=4)
        p.linear_colors = linear_colors
        buf.clear_frame()
        tb.render_with_params(network, p, buf.frame_buffer(), buf.depth_buffer())
        torch.cuda.synchronize()
        return buf.frame_buffer().clone()

    ds = runtime.Dataset(ctx, 8, W, H)
    origins = []
    for k in range(8):
        camera = synth.orbit_camera(45.0 * k, scale=cam_scale)
        origins.append(np.asarray(camera[9:12], np.float64))
        frame = render(tb.nerf_network, camera)
        assert float(frame[..., 3].max()) > 0.5, "the teacher's view shows the scene"
        ds.set_image(k, frame.contiguous())
        cam = _abi.TrainingCamera()
        cam.xform_start[:] = cam.xform_end[:] = camera.tolist()
        focal = 0.5 * W / math.tan(0.5 * synth.CAMERA_ANGLE_X)
        cam.focal_length[:], cam.principal_point[:] = (focal, focal), (0.5, 0.5)
        ds.set_camera(k, cam)
    origins = np.asarray(origins)
    assert (np.abs(origins - 0.5).max(1) < 2.0).all() and (np.abs(origins - 0.5).max(1) > 0.5).all(), "inside the box, outside the unit cube"
    held_out = synth.orbit_camera(22.5, 35.0, scale=cam_scale)
    return tb, ds, grid, render, held_out, render(tb.nerf_network, held_out)


@pytest.fixture(scope="module")
def teacher4(ctx, desc4):
    return make_teacher4(ctx, desc4)


def test_fit_end_to_end_at_aabb_scale_4(ctx, desc4, teacher4):
    """test_gpu_dataset.py::test_fit_end_to_end moved to aabb_scale 4: Trainer(max_cascade=2, cone_angle_constant=1/256).fit for 64 steps of 1024 rays.  The loss
    falls (test_trainer's criterion) and the held-out view rendered from the EMA weights is closer to the teacher's than from the initial weights; the grid updates
    reach cascades 1 and 2 and leave cascades 3 and 4 as mark_untrained left them, and cells no camera sees stay negative.
    The Trainer's default loss compares sRGB-encoded colours (train_in_linear_colors 0), so the student's network holds sRGB colours and its views are rendered
    without linear_colors, which converts them; the teacher's synthetic colours are taken as linear ones.  Measured on an MI355X (profiles/training_large_scenes.md):
    0.1130 before, 0.0324 after 64 steps.  Rendered WITH linear_colors, as test_fit_end_to_end renders its student, the held-out error does not fall at this scale,
    after 64 steps or after 256 (0.0294 -> 0.0325 -> 0.0331): the scene fills the unit cube, every view is opaque, and the initial weights' grey fog read as a
    linear colour is already closer to the teacher's grey than a trained frame whose sRGB values are read as linear ones.  Like test_fit_end_to_end's, the student
    marches through the TEACHER's grid; what is left of the error after the fit is printed beside the figure through the trainer's own grid."""
    from nerfshop_amd import _abi, runtime
    from nerfshop_amd.trainer import Trainer
    tb, ds, grid, render, held_out, truth = teacher4
    trainer = Trainer(ctx, desc4, seed=11, max_samples=1 << 17, max_cascade=2, cone_angle_constant=CONE)
    student = runtime.NerfNetwork(ctx, desc4, cell_cache_bytes=0)
    student.set_density_grid(grid)

    def held_out_error():
        student.set_params_device(trainer.optimizer.export_fp16(_abi.OPT_EXPORT_EMA))
        return float(((render(student, held_out, linear_colors=0) - truth) ** 2).mean())

    before = held_out_error()
    losses = trainer.fit(ds, 64, n_rays=1024)
    torch.cuda.synchronize()
    assert trainer.training_step == 64 and trainer.optimizer.step_count() == 64 and trainer.n_rays_total == 64 * 1024
    losses = [float(v) for v in losses]
    after = held_out_error()
    print("fit losses at aabb_scale 4:", " ".join(f"{v:.5f}" for v in losses))
    print(f"held-out view, mean squared error against the teacher: {before:.6f} before, {after:.6f} after")
    student.set_density_grid(np.maximum(trainer.network.get_density_grid(), 0.0))
    print(f"held-out view through the trainer's own grid: {held_out_error():.6f} after")
    assert len(losses) == 64 and all(np.isfinite(losses)) and losses[0] > 0
    assert np.mean(losses[-8:]) < np.mean(losses[:8])
    assert after < before
    # the grid: what mark_untrained leaves of a grid (0 where a camera sees the cell, -1 elsewhere, in all five cascades) on a second model, against the trainer's
    marked = runtime.NerfNetwork(ctx, desc4, cell_cache_bytes=0)
    marked.set_density_grid(np.zeros(_abi.GRID_VOLUME * _abi.GRID_CASCADES, np.float32))
    ds.mark_untrained(marked, clear_visible=True)
    want = marked.get_density_grid().reshape(_abi.GRID_CASCADES, -1)
    got = trainer.network.get_density_grid().reshape(_abi.GRID_CASCADES, -1)
    positive = [(int((c > 0).sum())) for c in got]
    print(f"density grid after the fit: positive cells per cascade {positive}, untrained cells per cascade {[int((c < 0).sum()) for c in got]}")
    assert (want < 0).any() and (want == 0).any()
    assert positive[1] > 0 and positive[2] > 0, "the grid updates reach cascades 1 and 2"
    assert got[3:].tobytes() == want[3:].tobytes(), "cascades above max_cascade are as mark_untrained left them"
    assert (got[:3][want[:3] < 0] < 0).all(), "cells no camera sees stay untrained through the grid updates"
    student.close(); marked.close()
