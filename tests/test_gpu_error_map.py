"""The training error map on the GPU against the twin of tests/error_map_ref.py: the deposits (cells integer-equal), the CDFs (bit-equal to the library's host twin,
which tests/test_error_map_host.py holds to the numpy twin), the rays drawn from them (pixels, xy and pdf bit-equal; jitter and background untouched), refusals and
states, and Trainer.fit with an ErrorMapSchedule.  Nothing here has a tolerance: the cells are integers, and every float compared is a chain of single IEEE operations
on the same inputs in the same order."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import dataset_ref
import error_map_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 1337
f32 = np.float32


@pytest.fixture(scope="module")
def ctx(built):
    from nerfshop_amd import runtime
    return runtime.Context(0)


def orbit_record(azimuth, width):
    from nerfshop_amd import synth
    start = np.asarray(synth.orbit_camera(azimuth), f32).reshape(4, 3).T
    end = np.asarray(synth.orbit_camera(azimuth + 7.0, 33.0), f32).reshape(4, 3).T
    focal = 0.5 * width / math.tan(0.5 * synth.CAMERA_ANGLE_X)
    return dataset_ref.camera_record(start, end, (focal, focal * 1.1), (0.47, 0.55), (0.1, 0.3, -0.2, 0.25))


def make_dataset(ctx, n_images, W, H, seed=3):
    from nerfshop_amd import runtime
    images = np.random.default_rng(seed).random((n_images, H, W, 4)).astype(np.float16)
    ds = runtime.Dataset(ctx, n_images, W, H)
    for k in range(n_images):
        ds.set_image(k, images[k])
        ds.set_camera(k, dataset_ref.to_struct(orbit_record(25.0 + 40.0 * k, W)))
    return ds, images


def heavy_tail(shape, seed):
    return (np.random.default_rng(seed).pareto(0.7, shape) * 1e-4).astype(f32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and (a.view(np.uint32) == b.view(np.uint32)).all()


def cells_of(ds):
    from nerfshop_amd import _abi
    return [int(c) for c in ds.error_map_get(_abi.ERROR_MAP_CELLS).tolist()]


# ---- accumulate -----------------------------------------------------------------------------------------------------------------------------------------------------
def accumulate_inputs(n_rays, n_images, seed, one_pixel=False, specials=True):
    """slots in a random order of the rays; losses with the special values in among ordinary ones; xy with both edges; a pdf between 0.1 and 60"""
    rng = np.random.default_rng(seed)
    ray_indices = rng.permutation(n_rays).astype(np.int32)
    loss = (rng.random(n_rays) * 0.3 / n_rays).astype(f32)
    if specials and n_rays >= 63:
        for k, v in enumerate((0.0, np.nan, -0.25, 1e9, 2.0 ** -34 / n_rays, np.inf, 2.0 ** -30 / n_rays)):
            if k * 9 < n_rays:
                loss[(k * 9) % n_rays] = v
    xy = rng.random((n_rays, 2)).astype(f32)
    xy[: min(n_rays, 4)] = np.array([[0.0, 0.0], [0.99999994, 0.99999994], [0.0, 0.99999994], [0.5, 0.5]], f32)[: min(n_rays, 4)]
    pixels = np.stack([rng.integers(0, n_images, n_rays), rng.integers(0, 64 * 48, n_rays)], 1).astype(np.int32)
    if one_pixel:
        xy[:], pixels[:] = (0.3210, 0.6540), (n_images - 1, 77)
    pdf = (0.1 + 59.9 * rng.random(n_rays)).astype(f32)
    return ray_indices, loss, xy, pixels, pdf


def run_accumulate(ds, shape, n_rays, counter, inputs, use_pdf, alias):
    ray_indices, loss, xy, pixels, pdf = inputs
    t = [torch.from_numpy(a).to(DEV) for a in (ray_indices, loss, xy, pixels, pdf)]
    cnt = torch.tensor([counter], dtype=torch.int32, device=DEV)
    weighted = t[1] if alias else torch.full((n_rays,), -7.0, dtype=torch.float32, device=DEV)
    ds.error_map_reset(shape[2], shape[1])
    ds.error_map_accumulate(n_rays, cnt, t[0], t[1], t[2], t[3], pdf=t[4] if use_pdf else None, loss_weighted=weighted)
    torch.cuda.synchronize()
    return cells_of(ds), weighted.cpu().numpy()


@pytest.fixture(scope="module")
def plain_datasets(ctx):
    """64 x 48 images that are never set: the map's calls need none"""
    from nerfshop_amd import runtime
    sets = {n: runtime.Dataset(ctx, n, 64, 48) for n in (1, 3)}
    yield sets
    for ds in sets.values():
        ds.close()


@pytest.mark.parametrize("n_images", [1, 3])
@pytest.mark.parametrize("res", [(2, 2), (5, 3), (29, 29)])
def test_accumulate(plain_datasets, res, n_images):
    ds = plain_datasets[n_images]
    shape = (n_images, res[1], res[0])
    n_cells = n_images * res[0] * res[1]
    for n_rays in (1, 63, 64, 65, 1000, 4096):
        for use_pdf, alias, counter in ((True, False, n_rays), (False, True, n_rays), (True, True, max(n_rays * 2 // 3, 1)), (False, False, n_rays + 5)):
            inputs = accumulate_inputs(n_rays, n_images, seed=n_rays + 7 * n_images)
            got, weighted = run_accumulate(ds, shape, n_rays, counter, inputs, use_pdf, alias)
            want = [0] * n_cells
            want_weighted = ref.accumulate(want, shape, n_rays, counter, *inputs[:4], pdf=inputs[4] if use_pdf else None)
            where = (res, n_images, n_rays, use_pdf, alias, counter)
            assert got == want, where
            live = min(counter, n_rays)
            assert same_bits(weighted[:live], want_weighted), where
            if alias and not use_pdf:
                assert same_bits(weighted, inputs[1]), "without a pdf the losses keep their bits, NaN and -0 included"
            assert same_bits(weighted[live:], inputs[1][live:] if alias else np.full(n_rays - live, -7.0, f32)), "slots past the counter are left alone"
            if n_rays >= 64:
                assert sum(want) > 0 and sum(1 for c in want if c) >= min(4, n_cells)
    again, _ = run_accumulate(ds, shape, 4096, 4096, accumulate_inputs(4096, n_images, seed=4096 + 7 * n_images), True, False)
    inputs = accumulate_inputs(4096, n_images, seed=4096 + 7 * n_images)
    first, _ = run_accumulate(ds, shape, 4096, 4096, inputs, True, False)
    assert again == first, "a second run gives the same bits"


@pytest.mark.parametrize("res", [(2, 2), (29, 29)])
def test_accumulate_one_pixel(plain_datasets, res):
    """all 4096 rays on one pixel: four cells take every atomic, and the sum does not depend on their order"""
    ds, n_images, n_rays = plain_datasets[3], 3, 4096
    shape = (n_images, res[1], res[0])
    inputs = accumulate_inputs(n_rays, n_images, seed=5, one_pixel=True, specials=False)
    got, _ = run_accumulate(ds, shape, n_rays, n_rays, inputs, True, False)
    want = [0] * (n_images * res[0] * res[1])
    ref.accumulate(want, shape, n_rays, n_rays, *inputs[:4], pdf=inputs[4])
    assert got == want and sum(1 for c in want if c) == 4
    # the clamp value 2^21 times over fits: 4096 deposits of 1e9 (clamped to 1024) into one corner cell
    inputs = list(inputs)
    inputs[1] = np.full(n_rays, 1e9, f32)
    inputs[2] = np.zeros((n_rays, 2), f32)
    got, _ = run_accumulate(ds, shape, n_rays, n_rays, inputs, False, False)
    assert got[2 * res[0] * res[1]] == n_rays << 42 and sum(got) == n_rays << 42


# ---- the CDFs -------------------------------------------------------------------------------------------------------------------------------------------------------
CDF_SHAPES = [(1, 2, 2), (3, 3, 5), (7, 29, 29), (2, 2, 1024), (2, 1024, 2), (3, 5, 63), (3, 5, 64), (3, 5, 65), (2, 3, 256), (100, 29, 29), (1025, 3, 17), (130, 2, 2)]


@pytest.mark.parametrize("shape", CDF_SHAPES)
def test_build_cdfs(ctx, shape):
    """a dataset whose images have the map's resolution (the largest map it accepts); set -> build -> get against the host twin on the float map as the library
    reads it.  (130, 2, 2): more than 64 pictures with more than 64 x 2 rows in all -- every stage of the build runs more than one block."""
    from nerfshop_amd import _abi, runtime
    n, res_y, res_x = shape
    ds = runtime.Dataset(ctx, n, res_x, res_y)
    rng = np.random.default_rng(n + res_x)
    maps = {"zero": np.zeros(shape, f32), "heavy_tail": heavy_tail(shape, n + res_y)}
    for name, x in (("spike_first", 0), ("spike_last", res_x - 1)):
        m = (rng.random(shape) * 1e-3).astype(f32)
        m[n - 1, res_y // 2, x] = 1e6
        maps[name] = m
    for name, m in maps.items():
        ds.error_map_set(m)
        data = ds.error_map_get(_abi.ERROR_MAP_FLOAT).reshape(shape)
        assert same_bits(data, ref.cells_to_float(ref.quantise(m)).reshape(shape)), "set quantises by the deposit rule"
        ds.error_map_build_cdfs()
        want = runtime.error_map_cdfs_host(data)
        for what, w in zip((_abi.ERROR_MAP_CDF_X_COND_Y, _abi.ERROR_MAP_CDF_Y, _abi.ERROR_MAP_CDF_IMG, _abi.ERROR_MAP_PMF_IMG), want):
            assert same_bits(ds.error_map_get(what), w.reshape(-1)), (shape, name, what)
    ds.close()


# ---- rays drawn from the CDFs ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ray_datasets(ctx):
    sets = {n: make_dataset(ctx, n, 64, 48, seed=n) for n in (3, 7)}
    yield sets
    for ds, _ in sets.values():
        ds.close()


def gpu_rays(ds, n_rays, total, snap, by_error):
    out = ds.rays(n_rays, total, dataset_ref.rng_of(SEED), snap=snap, random_bg=True, by_error=by_error)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


@pytest.mark.parametrize("n_images", [3, 7])
def test_rays_ex_flags_off(ray_datasets, n_images):
    """bit-equal to nrs_dataset_rays in every output they share, pdf exactly 1, xy the snapped position -- with and without CDFs in the dataset"""
    ds, images = ray_datasets[n_images]
    for n_rays in (1, 64, 65, 1000, 4096):
        for total in (0, ((1 << 32) // n_images - max(n_rays // 2, 1)) & 0xffffffff):
            for snap in (True, False):
                plain = gpu_rays(ds, n_rays, total, snap, None)
                ex = gpu_rays(ds, n_rays, total, snap, (False, False))
                assert all(same_bits(a, b) for a, b in zip(plain, ex[:5])), (n_rays, total, snap)
                assert (ex[6] == 1).all()
                W, H = 64, 48
                px, py = np.clip((ex[5][:, 0] * f32(W)).astype(np.int32), 0, W - 1), np.clip((ex[5][:, 1] * f32(H)).astype(np.int32), 0, H - 1)
                assert ((px + py * W) == plain[4][:, 1]).all()


@pytest.mark.parametrize("n_images", [3, 7])
@pytest.mark.parametrize("cdf_res", [(29, 29), (64, 48), (2, 2)])
def test_rays_ex_by_error(ray_datasets, cdf_res, n_images):
    """Every flag combination over every shape, none left out of any comparison.  The tables the twin searches are the ones the GPU built (test_build_cdfs holds them to
    the host twin).  cdf_res (64, 48) is the image's own resolution, (2, 2) the smallest map."""
    from nerfshop_amd import _abi
    ds, images = ray_datasets[n_images]
    W, H = 64, 48
    shape = (n_images, cdf_res[1], cdf_res[0])
    ds.error_map_set(heavy_tail(shape, 11 + n_images))
    ds.error_map_build_cdfs()
    tables = (ds.error_map_get(_abi.ERROR_MAP_CDF_X_COND_Y).reshape(shape), ds.error_map_get(_abi.ERROR_MAP_CDF_Y).reshape(shape[:2]), ds.error_map_get(_abi.ERROR_MAP_CDF_IMG))
    seen_imgs, moved = set(), 0
    for n_rays in (1, 64, 65, 1000, 4096):
        draws = dataset_ref.draws(SEED, n_rays)
        for total in (0, 12345, ((1 << 32) - n_rays // 2) & 0xffffffff):   # the last: i + n_rays_total wraps inside the batch
            for snap in (True, False):
                off = gpu_rays(ds, n_rays, total, snap, (False, False))
                for by_images, by_pixels in ((False, True), (True, False), (True, True)):
                    rays, jitter, target, background, pixels, xy, pdf = gpu_rays(ds, n_rays, total, snap, (by_images, by_pixels))
                    want = ref.sample(SEED, n_rays, total, n_images, W, H, snap, tables, by_images, by_pixels)
                    where = (cdf_res, n_images, n_rays, total, snap, by_images, by_pixels)
                    assert (pixels[:, 0].view(np.uint32) == want["img"]).all(), where
                    assert (pixels[:, 1].view(np.uint32) == want["pixel"]).all(), where
                    assert same_bits(xy, want["xy"]) and same_bits(pdf, want["pdf"]), where
                    assert same_bits(jitter, off[1]) and same_bits(background, off[3]), "no draw is added or moved"
                    py, px = pixels[:, 1] // W, pixels[:, 1] % W
                    assert same_bits(target, images[pixels[:, 0], py, px].astype(f32)), where
                    assert np.isfinite(rays).all() and np.allclose(np.linalg.norm(rays[:, 3:], axis=1), 1.0, atol=1e-5), where
                    if by_pixels and not by_images:
                        assert not ((pdf != 1) & (draws[:, 0] < f32(0.5))).any(), "pdf != 1 only where draw 0 >= 0.5"
                        assert same_bits(pdf[want["cdf_half"]], want["pdf"][want["cdf_half"]])
                        moved += int((pixels[:, 1] != off[4][:, 1]).sum())
                    if not by_pixels:
                        assert same_bits(xy, off[5]), where
                    if by_images:
                        seen_imgs |= set(pixels[:, 0].tolist())
    assert seen_imgs == set(range(n_images)) and moved > 1000, "the switches do something"


# ---- refusals and states --------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_states(ctx):
    from nerfshop_amd import _abi, runtime
    from nerfshop_amd._abi import NrsError
    ds = runtime.Dataset(ctx, 2, 1100, 3)
    rng = dataset_ref.rng_of(SEED)
    q = torch.zeros(64, dtype=torch.int32, device=DEV)
    qf = torch.zeros(64, dtype=torch.float32, device=DEV)
    for what in (_abi.ERROR_MAP_FLOAT, _abi.ERROR_MAP_CELLS):
        with pytest.raises(NrsError, match="error -5.*no map"):
            ds.error_map_get(what)
    with pytest.raises(NrsError, match="error -5.*no map"):
        ds.error_map_accumulate(8, q, q, qf, qf, q)
    with pytest.raises(NrsError, match="error -5.*no map"):
        ds.error_map_build_cdfs()
    for res in ((1, 2), (2, 1), (0, 0), (2, 4), (1101, 2), (1025, 2)):   # below 2; past the image's 3 rows; past the image's width; past 1024
        with pytest.raises(NrsError, match="error -1.*resolution"):
            ds.error_map_reset(*res)
        with pytest.raises(NrsError, match="error -1.*resolution"):
            ds.error_map_set(np.zeros((2, res[1], res[0]), f32))
    ds.error_map_reset(1024, 3)
    assert ds.error_map_get(_abi.ERROR_MAP_CELLS).shape == (2 * 3 * 1024,) and not ds.error_map_get().any()
    for what in (_abi.ERROR_MAP_CDF_X_COND_Y, _abi.ERROR_MAP_CDF_Y, _abi.ERROR_MAP_CDF_IMG, _abi.ERROR_MAP_PMF_IMG):
        with pytest.raises(NrsError, match="error -5.*no valid CDFs"):
            ds.error_map_get(what)
    with pytest.raises(NrsError, match="error -1.*unknown"):
        ds.error_map_get(6)
    lib = ctx.lib
    p = q.data_ptr()
    assert lib.nrs_dataset_error_map_accumulate(ds.h, None, (1 << 21) + 1, p, p, p, p, p, None, None) == -1 and b"2^21" in lib.nrs_last_error()   # (refused before it reads a thing)
    for args in ((None, p, p, p, p), (p, None, p, p, p), (p, p, None, p, p), (p, p, p, None, p), (p, p, p, p, None)):
        assert lib.nrs_dataset_error_map_accumulate(ds.h, None, 8, *args, None, None) == -1
    with pytest.raises(NrsError):
        ds.error_map_accumulate(8, q.cpu(), q, qf, qf, q)   # a host tensor never reaches the library
    ds.error_map_accumulate(0, q, q, qf, qf, q)
    # rays_ex: an incomplete dataset; a switch without CDFs; the struct size; too many rays
    with pytest.raises(NrsError, match="error -5.*image has never been set"):
        ds.rays(8, 0, rng, by_error=(False, False))
    ds.close()
    ds, _ = make_dataset(ctx, 2, 16, 12)
    for flags in ((True, False), (False, True), (True, True)):
        with pytest.raises(NrsError, match="error -5.*without valid CDFs"):
            ds.rays(8, 0, rng, by_error=flags)
    assert ds.rays(0, 0, rng, by_error=(False, False))[5].shape == (0, 2)
    with pytest.raises(NrsError, match="2\\^21"):
        ds.rays((1 << 21) + 1, 0, rng, by_error=(False, False))
    bad = _abi.DatasetRaysExParams()
    bad.struct_size = C.sizeof(_abi.DatasetRaysParams)
    pf = qf.data_ptr()
    assert lib.nrs_dataset_rays_ex(ds.h, None, C.byref(bad), 1, pf, pf, pf, pf, p, pf, pf) == -1
    good = _abi.DatasetRaysExParams()
    assert lib.nrs_dataset_rays_ex(ds.h, None, C.byref(good), 1, None, pf, pf, pf, p, pf, pf) == -1
    assert lib.nrs_dataset_rays_ex(ds.h, None, C.byref(good), 1, pf, pf, pf, pf, None, None, None) == 0, "pixels, xy and pdf may be NULL"
    # valid CDFs carry their own resolution and survive a reset of the map to another one
    ds.error_map_set(heavy_tail((2, 5, 7), 1))
    ds.error_map_build_cdfs()
    before = [ds.error_map_get(w) for w in (1, 2, 3, 4)]
    first = [t.cpu().numpy() for t in ds.rays(1000, 0, rng, by_error=(True, True))]
    ds.error_map_reset(3, 2)
    assert ds.error_map_get(_abi.ERROR_MAP_CELLS).shape == (12,) and before[0].shape == (70,)
    assert all(same_bits(a, ds.error_map_get(w)) for a, w in zip(before, (1, 2, 3, 4)))
    again = [t.cpu().numpy() for t in ds.rays(1000, 0, rng, by_error=(True, True))]
    assert all(same_bits(a, b) for a, b in zip(first, again))
    ds.error_map_build_cdfs()
    assert ds.error_map_get(_abi.ERROR_MAP_CDF_X_COND_Y).shape == (12,), "a build takes the map's resolution"
    torch.cuda.synchronize()
    ds.close()


# ---- the trainer ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def desc14():
    from nerfshop_amd import synth
    return synth.model_desc(log2_hashmap_size=14)


@pytest.fixture(scope="module")
def fit_rig(ctx, desc14):
    """8 views of 32 x 32 random pixels, 1024 rays a step: fit(schedule, n_steps, learning_rate) -> (trainer, the losses as float32)"""
    from nerfshop_amd import _abi, synth
    from nerfshop_amd.trainer import Trainer
    ds, _ = make_dataset(ctx, 8, 32, 32, seed=21)
    grid = synth.density_grid(1)

    def fit(schedule, n_steps, learning_rate=_abi.BASE_LEARNING_RATE):
        trainer = Trainer(ctx, desc14, seed=11, density_grid=grid, max_samples=1 << 17, learning_rate=learning_rate)
        losses = trainer.fit(ds, n_steps, n_rays=1024, error_map=schedule) if schedule is not None else trainer.fit(ds, n_steps, n_rays=1024)
        torch.cuda.synchronize()
        return trainer, np.array([float(v) for v in losses], f32)
    yield ds, fit
    ds.close()


def first_difference(a, b):
    d = np.flatnonzero(a.view(np.uint32) != b.view(np.uint32))
    return int(d[0]) + 1 if d.size else None


def test_fit_observes_and_does_not_steer(fit_rig):
    """fit with ErrorMapSchedule(steps_between=4) and both switches off returns the losses of fit without it, bit for bit, over 19 steps: three builds, three maps of
    three resolutions, two grid updates.

    The comparison is made at learning rate 0.  Two fits WITHOUT a schedule do not return the same bits at the default learning rate, before this feature or after
    it: the backward pass sums parameter gradients with float atomics ("The backward pass": "the last bits depend on the order of arrival"), so from the
    second step on the weights, and with them every later loss, carry the order in which the adds arrived.  Measured on an MI355X with this file's rig: two plain fits
    first differ at step 5 or 6 of 19 (one float32 step), a plain fit and a fit with the schedule at step 4 or 5 -- the same noise.  At learning rate 0 Adam leaves
    every weight where it is, fit is a function of its inputs (asserted first: two plain fits agree in every bit), each step still draws its own rays, and any
    way in which the schedule could steer -- other rays, another jitter or background, a loss buffer rewritten before the sum -- shows in the loss.  The figures at
    the default learning rate are printed, with no bar."""
    from nerfshop_amd import _abi
    from nerfshop_amd.trainer import ErrorMapSchedule
    ds, fit = fit_rig
    _, plain = fit(None, 19, 0.0)
    _, plain_again = fit(None, 19, 0.0)
    assert np.isfinite(plain).all() and plain[0] > 0 and len(set(plain.tolist())) == 19
    assert same_bits(plain, plain_again), "at learning rate 0 fit is a function of its inputs"
    observed = ErrorMapSchedule(steps_between=4)
    _, with_map = fit(observed, 19, 0.0)
    assert same_bits(plain, with_map), f"first differing step: {first_difference(plain, with_map)}"
    assert observed.build_steps == [4, 10, 19] and observed.builds == 3 and observed.steps_between == 13
    assert ds.error_map_get(_abi.ERROR_MAP_CELLS).any(), "and it did observe"
    _, a = fit(None, 19)
    _, b = fit(None, 19)
    _, c = fit(ErrorMapSchedule(steps_between=4), 19)
    print(f"default learning rate, first differing step of 19: plain against plain {first_difference(a, b)}, plain against a fit with the schedule {first_difference(a, c)}")
    assert same_bits(a[:1], b[:1]) and same_bits(a[:1], c[:1]), "the first step's loss is computed before any backward pass"


def test_fit_with_a_schedule(fit_rig):
    """The CDFs are built after steps 4, 10 and 19 (4, then 6, then 9 steps between).  With both switches on the losses stay finite, and the map read back after the
    step that follows a build is the twin's accumulate of that step's loss, xy, pixels and pdf."""
    from nerfshop_amd import _abi
    from nerfshop_amd.trainer import ErrorMapSchedule
    ds, fit = fit_rig
    n_rays = 1024
    observed = ErrorMapSchedule(steps_between=4)
    _, losses = fit(observed, 19)
    assert np.isfinite(losses).all() and observed.build_steps == [4, 10, 19] and observed.steps_between == 13 and observed.builds == 3
    assert observed.resolution == (20, 20), "the map of step 11, with 9 steps between: (9 * 1024 / 8) ^ (1 / 4) * 3.5 = 20.4"
    assert ds.error_map_get(_abi.ERROR_MAP_CDF_IMG).shape == (8,) and ds.error_map_get(_abi.ERROR_MAP_CDF_Y).shape == (8 * 20,)

    steered = ErrorMapSchedule(steps_between=4, sample_images=True, sample_pixels=True, keep_last=True)
    trainer, losses = fit(steered, 10)
    assert np.isfinite(losses).all() and (losses > 0).all() and steered.build_steps == [4, 10] and steered.steps_since == 0
    loss = trainer.step_dataset(ds, n_rays, error_map=steered)   # step 11: a fresh map at the recomputed resolution, one step's deposits
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and steered.resolution == (20, 20) and steered.steps_between == 9
    counter, ray_indices, slot_loss = [t.cpu().numpy() for t in steered.last_loss]
    xy, pixels, pdf = [t.cpu().numpy() for t in steered.last_rays]
    shape = (8, steered.resolution[1], steered.resolution[0])
    want = [0] * (shape[0] * shape[1] * shape[2])
    weighted = ref.accumulate(want, shape, n_rays, int(counter[0]), ray_indices, slot_loss, xy, pixels, pdf=pdf)
    assert cells_of(ds) == want and sum(want) > 0
    assert (pdf != 1).any() and len(set(pixels[:, 0].tolist())) == 8 and np.isfinite(weighted).all(), "the step was steered"
    total = float(np.concatenate([weighted, slot_loss[len(weighted):]]).astype(np.float64).sum())
    assert abs(float(loss) - total) < 1e-4 * abs(total), "the reported loss is the sum of loss / pdf"

