"""Per-image exposure on the GPU against tests/exposure_ref.py: nrs_exposure_targets, nrs_exposure_accumulate, nrs_exposure_step.

One batch shape for everything, tests/test_gpu_envmap.py's (its make_batch): 200 ray slots (not a multiple of 64 or 256) of 0..130 samples (rays the opaque samples
stop, rays of more than 64 samples), 187 of them below the counter, a compact buffer 150 samples short of what they consume (the last rays keep no sample: M' = 0),
two rays without samples, slots in a permuted order of the rays.  Five assignments of images to SLOTS (the wave's view; a ray's image follows from its slot):
  (a) one image;  (b) three images of five in runs whose boundaries (slots 40 and 150) fall inside waves;  (c) five images interleaved lane by lane: every wave
  peels five times;  (d) 70 images, slot s on image s % 70: a wave of 64 distinct images, more images than lanes across the batch;  (e) as (b), with one live ray on
  image n_images and one live slot whose ray index is n_rays + 5.

Bars.  The scale against float64 exp2 within 1e-5 relative (test_gpu_ray_loss' bar for a per-ray quantity).  d_target_out: bit for bit scale * rgb at the device's
own scale.  The cells: the twin's integers from the device's own aux and d_scale records, bit for bit under train_in_linear_colors; in sRGB (one powf, in the
divisor) the float gradient against the float64 evaluation on the device's records, per cell relative to the magnitudes deposited there, 1e-6: the bar
tests/test_gpu_envmap.py states for its sRGB cells, whose divisor holds two powf.  The step: test_gpu_optimizer's bars -- against the float64 twin at most 4 x the
float32 twin's error plus one float32 step -- and, as that file asserts for the optimiser's kernel, bit-equal to the same fp32 operations on the host, here
nrs_exposure_step_host on the downloaded state."""
import ctypes as C

import numpy as np
import pytest
import torch

import envmap_ref
import exposure_ref as ref
import optimizer_ref
import ray_loss_ref as rl
from test_gpu_envmap import LIVE, R, loss_buffers, loss_params, make_batch, t, upload

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
CLIP = 150
CASES = ["one", "runs", "interleaved", "seventy", "out_of_range"]


@pytest.fixture(scope="module")
def ctx(built):
    from nerfshop_amd import runtime
    return runtime.Context(0)


@pytest.fixture(scope="module")
def net(ctx):
    from nerfshop_amd import runtime, synth
    desc = synth.model_desc(1, log2_hashmap_size=14)
    desc.rgb_activation, desc.density_activation = rl.ACT_LOGISTIC, rl.ACT_EXPONENTIAL
    return runtime.NerfNetwork(ctx, desc, cell_cache_bytes=0)


def assignment(case, idx):
    """-> (n_images, image by RAY [R] uint32, ray_indices [R]) of one case; idx: the batch's permutation (slot -> ray)"""
    s = np.arange(R)
    idx = idx.copy()
    if case == "one":
        n_images, by_slot = 1, np.zeros(R, np.int64)
    elif case in ("runs", "out_of_range"):
        n_images, by_slot = 5, np.where(s < 40, 0, np.where(s < 150, 2, 4))
    elif case == "interleaved":
        n_images, by_slot = 5, s % 5
    else:
        n_images, by_slot = 70, s % 70
    by_ray = np.zeros(R, np.uint32)
    by_ray[idx] = by_slot
    if case == "out_of_range":
        by_ray[idx[20]] = n_images      # a live ray on an image that does not exist
        idx[30] = R + 5                 # a live slot that names no ray
    return n_images, by_ray, idx


def exposures_for(n_images, seed=9):
    return np.random.default_rng(seed + n_images).uniform(-1.5, 1.5, (n_images, 3)).astype(f32)


class Run:
    pass


def pipeline(ctx, net, b, case, pdf=False, accumulate=True, exposure=None, n_images=None):
    """targets -> ray_loss(aux) -> accumulate on a fresh exposure (or on `exposure`); everything the checks need, on the host"""
    from nerfshop_amd import _abi, runtime
    r = Run()
    r.n_images, r.img, r.idx = assignment(case, b["ray_indices"])
    bb = dict(b, ray_indices=r.idx.astype(np.int32))
    u = upload(bb)
    r.values = exposures_for(r.n_images)
    if exposure is None:
        exposure = runtime.Exposure(ctx, r.n_images)
        exposure.set(r.values)
    r.exp, r.u = exposure, u
    pixels = np.stack([r.img, np.arange(R, dtype=np.uint32) * 3 + 1], 1)
    r.pixels = t(pixels.view(np.int32), torch.int32)
    r.pdf = np.random.default_rng(4).uniform(0.25, 4.0, R).astype(f32) if pdf else None
    r.d_pdf = None if r.pdf is None else t(r.pdf, torch.float32)
    target_out = torch.full((R, 4), float("nan"), dtype=torch.float32, device=DEV)
    scale = torch.full((R, 4), -1, dtype=torch.int32, device=DEV)
    aux = torch.full((R, 12), -7, dtype=torch.int32, device=DEV)
    exposure.targets(u.ray_indices, u.counter, r.pixels, u.target, out=(target_out, scale))
    outs = net.ray_loss(None, loss_params(b), u.numsteps, u.coords, u.out16, target_out, background=u.bg, ray_counter=u.counter, out=loss_buffers(b), aux=aux)
    p = b["p"]
    r.acc = _abi.ExposureAccumulateParams(p["loss_scale"], int(p["lin"]))
    r.d = (target_out, scale, aux, outs[0])
    if accumulate:
        exposure.accumulate(r.acc, u.counter, u.ray_indices, outs[0], aux, scale, xy_pdf=r.d_pdf, n_rays=R)
    torch.cuda.synchronize()
    r.target_out, r.scale, r.aux_words, r.numsteps_out = target_out.cpu().numpy(), scale.cpu().numpy(), aux.cpu().numpy(), outs[0].cpu().numpy()
    r.aux = envmap_ref.split_aux(r.aux_words)
    r.cells = exposure.get(_abi.EXPOSURE_CELLS) if accumulate else None
    return r


def want_cells(b, r, cells=None):
    return ref.accumulate_cells(R, r.n_images, LIVE, r.idx, r.numsteps_out, r.aux, r.scale, r.pdf, b["p"]["loss_scale"], bool(b["p"]["lin"]), cells=cells)


def as_ints(cells):
    return [int(c) for c in np.asarray(cells).reshape(-1)]


def depositing(r):
    return ref.deposits(R, r.n_images, LIVE, r.idx, r.numsteps_out, r.scale)


# ---- targets --------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_targets(ctx, net, case):
    b = make_batch(loss_type=rl.L2, lin=True, clip=CLIP)
    r = pipeline(ctx, net, b, case, accumulate=False)
    skipped = ref.skipped(R, r.n_images, LIVE, r.idx, np.stack([r.img, r.img], 1))
    assert skipped.sum() == (R - LIVE) + (2 if case == "out_of_range" else 0)
    assert np.isnan(r.target_out[skipped]).all() and (r.scale[skipped] == -1).all(), "a skipped slot, and one at or past the counter, is not written"
    ok = ~skipped
    words = r.scale.view(np.uint32)
    img = r.img[r.idx[ok]]
    assert (words[ok, 3] == img).all(), "the record names the slot's image"
    scale = words[:, :3].copy().view(f32)
    want = ref.scale64(r.values)[img]
    rel = np.abs(scale[ok].astype(np.float64) - want) / want
    print(f"{case}: scale against float64 exp2 {rel.max():.3e} relative (bar 1e-5)")
    assert rel.max() <= 1e-5
    got = r.target_out[ok]
    assert got.tobytes() == ref.targets(scale[ok], r.idx[ok], b["target"]).tobytes(), "(scale * rgb, a), each product rounded once, at the device's own scale"
    assert (got[:, 3] == b["target"][r.idx[ok], 3]).all()
    assert len(set(img.tolist())) == {"one": 1, "runs": 3, "interleaved": 5, "seventy": 70, "out_of_range": 3}[case]


def test_fresh_exposures_are_zero_and_scale_one(ctx, net):
    """A fresh handle: zero exposures, so every scale is exactly 1 and the targets are the gather; export and get agree; set(None) and set(values) reset the state."""
    from nerfshop_amd import _abi, runtime
    b = make_batch(loss_type=rl.L2, lin=True, clip=CLIP)
    u = upload(b)
    exp = runtime.Exposure(ctx, 3)
    assert exp.n_images == 3 == exp.lib.nrs_exposure_n_images(exp.h) and exp.step_count() == 0
    for which in (_abi.EXPOSURE_VALUES, _abi.EXPOSURE_M, _abi.EXPOSURE_V, _abi.EXPOSURE_CELLS, _abi.EXPOSURE_GRADIENT):
        assert not exp.get(which).any()
    pixels = t(np.stack([np.arange(R) % 3, np.arange(R)], 1).astype(np.int32), torch.int32)
    target, scale = exp.targets(u.ray_indices, u.counter, pixels, u.target)
    torch.cuda.synchronize()
    assert target.cpu().numpy()[:LIVE].tobytes() == b["target"][b["ray_indices"][:LIVE]].tobytes()
    assert (scale.cpu().numpy()[:LIVE, :3].view(f32) == 1.0).all() and not scale.cpu().numpy()[LIVE:].any() and not target.cpu().numpy()[LIVE:].any()
    values = exposures_for(3)
    exp.set(values)
    assert exp.get().tobytes() == values.tobytes() == exp.export().cpu().numpy().tobytes()
    exp.set(None)
    assert not exp.get().any()


# ---- accumulate, exact --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pdf", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_accumulate_cells_are_exact(ctx, net, case, pdf):
    """train_in_linear_colors: no powf between the records and the cells, so the cells are the twin's integers bit for bit -- one atomic per image, channel and wave
    leaves what one atomic per lane would leave.  Images without depositing rays stay zero; two identical calls give identical cells; a second accumulate adds."""
    from nerfshop_amd import _abi
    b = make_batch(loss_type=rl.L2 if pdf else rl.RELATIVE_L2, lin=True, clip=CLIP)
    r = pipeline(ctx, net, b, case, pdf=pdf)
    want = want_cells(b, r)
    got = as_ints(r.cells)
    assert got == want
    ok = depositing(r)
    live = np.arange(R) < LIVE
    stopped = live & (r.aux["M"] < r.aux["n"]) & (r.numsteps_out[:, 0] > 0)
    emptied = live & (r.aux["n"] > 0) & (r.numsteps_out[:, 0] == 0)
    assert ok.sum() >= 100 and (ok & stopped).sum() >= 5, "a stopped ray still deposits"
    assert emptied.sum() >= 1 and not (ok & emptied).any() and not (ok & (r.aux["n"] == 0)).any(), "rays the compact buffer leaves no sample, and rays without samples, do not"
    used = set(int(x) for x in r.scale.view(np.uint32)[ok, 3])
    if case == "seventy":
        assert len(used) > 64, "more distinct images than a wave has lanes"
    else:
        assert used == {"one": {0}, "runs": {0, 2, 4}, "interleaved": set(range(5)), "out_of_range": {0, 2, 4}}[case]
    cells = np.asarray(got, dtype=object).reshape(r.n_images, 3)
    for i in range(r.n_images):
        assert bool(cells[i].any()) == (i in used), "images without depositing rays stay zero; the others hold a gradient"
    again = pipeline(ctx, net, b, case, pdf=pdf)
    assert as_ints(again.cells) == got, "two identical calls give identical cells"
    r.exp.accumulate(r.acc, r.u.counter, r.u.ray_indices, r.d[3], r.d[2], r.d[1], xy_pdf=r.d_pdf, n_rays=R)
    assert as_ints(r.exp.get(_abi.EXPOSURE_CELLS)) == [2 * c for c in got] == want_cells(b, r, cells=want), "a second accumulate adds"
    assert (r.exp.get(_abi.EXPOSURE_GRADIENT).reshape(-1) == envmap_ref.cells_to_gradient([2 * c for c in got])).all()


def test_a_slot_without_a_ray_never_deposits(ctx, net):
    """(e) again, with valid records written under the two skipped slots by hand: the slot whose ray index is out of range still deposits nothing -- accumulate
    checks the index itself -- and the record of the other slot is read as it stands, as the header says."""
    from nerfshop_amd import _abi, runtime
    b = make_batch(loss_type=rl.L2, lin=True, clip=CLIP)
    r = pipeline(ctx, net, b, "out_of_range", accumulate=False)
    scale = r.d[1].clone()
    one = int(np.array([1.0], f32).view(np.int32)[0])
    scale[20] = torch.tensor([one, one, one, 1], dtype=torch.int32)
    scale[30] = torch.tensor([one, one, one, 1], dtype=torch.int32)
    aux = r.d[2].clone()
    aux[20, :3] = one          # a gradient of 1 per channel where the loss saw the canary
    aux[30, :3] = one
    r.exp.accumulate(r.acc, r.u.counter, r.u.ray_indices, r.d[3], aux, scale, n_rays=R)
    got = as_ints(r.exp.get(_abi.EXPOSURE_CELLS))
    a = envmap_ref.split_aux(aux.cpu().numpy())
    want = ref.accumulate_cells(R, r.n_images, LIVE, r.idx, r.numsteps_out, a, scale.cpu().numpy(), None, b["p"]["loss_scale"], True)
    assert got == want
    assert r.numsteps_out[20, 0] > 0 and r.numsteps_out[30, 0] > 0, "both slots hold samples"
    per_ray = envmap_ref.quantise(f32(f32(f32(f32(b["p"]["loss_scale"]) / f32(R)) * f32(-1.0)) * ref.LN2))
    assert got[3:6] == [per_ray] * 3, "image 1 holds slot 20's deposit alone: slot 30 names no ray"


def test_ray_count_refusal(ctx, net):
    """The call that would take the rays accumulated since the last step past 2^21 is refused with NRS_ERR_STATE, before anything is enqueued; a step resets the
    count."""
    from nerfshop_amd import _abi
    from nerfshop_amd.runtime._base import _stream_handle
    b = make_batch(loss_type=rl.L2, lin=True, clip=CLIP)
    r = pipeline(ctx, net, b, "runs")
    before = as_ints(r.cells)
    big = (1 << 21) - R + 1

    def call(n):
        return r.exp.lib.nrs_exposure_accumulate(r.exp.h, _stream_handle(None), C.byref(r.acc), n, r.u.counter.data_ptr(), r.u.ray_indices.data_ptr(), r.d[3].data_ptr(),
                                                 r.d[2].data_ptr(), r.d[1].data_ptr(), None)
    assert call(big) == -5 and "2^21" in r.exp.lib.nrs_last_error().decode()
    assert as_ints(r.exp.get(_abi.EXPOSURE_CELLS)) == before
    assert call(R) == 0, "a batch that fits is taken"
    assert call(big - R) == -5, "and counted"
    r.exp.step(loss_scale=b["p"]["loss_scale"], lr=1e-2)
    assert call(R) == 0 and call(big) == -5, "the step resets the count"
    r.exp.set(None)
    assert call(R) == 0 and call(big) == -5, "and so does set"


# ---- accumulate, sRGB ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("color_space", [rl.LINEAR, rl.SRGB])
@pytest.mark.parametrize("case", ["runs", "seventy"])
def test_accumulate_srgb_gradient(ctx, net, case, color_space):
    """Without train_in_linear_colors the divisor srgb_to_linear_derivative(target) holds one powf.  The float gradient against the float64 evaluation of the same
    expressions on the device's records, per cell relative to the sum of the magnitudes deposited there; the bar is tests/test_gpu_envmap.py's for its sRGB cells,
    1e-6."""
    from nerfshop_amd import _abi
    b = make_batch(loss_type=rl.L2, color_space=color_space, lin=False, clip=CLIP)
    r = pipeline(ctx, net, b, case, pdf=True)
    got = r.exp.get(_abi.EXPOSURE_GRADIENT).reshape(-1).astype(np.float64)
    assert (got == envmap_ref.cells_to_gradient(as_ints(r.cells)).astype(np.float64)).all(), "the gradient is the cells' own expression"
    ok = depositing(r)
    g, tg = r.aux["g"].astype(np.float64), r.aux["target"].astype(np.float64)
    deriv = np.where(tg <= 0.04045, 1.0 / 12.92, 2.4 / 1.055 * np.power((np.maximum(tg, 0.04045) + 0.055) / 1.055, 1.4))
    words = r.scale.view(np.uint32)
    sc = words[:, :3].copy().view(f32).astype(np.float64)
    pdf = np.ones(R)
    pdf[ok] = r.pdf[r.idx[ok]]
    v = (float(f32(b["p"]["loss_scale"])) / R) * (-g / pdf[:, None]) / deriv * sc * float(ref.LN2)
    want, size = np.zeros(3 * r.n_images), np.zeros(3 * r.n_images)
    for s in np.nonzero(ok)[0]:
        for c in range(3):
            want[3 * int(words[s, 3]) + c] += v[s, c]
            size[3 * int(words[s, 3]) + c] += abs(v[s, c])
    assert (np.abs(v[ok]) < 512).all() and (size > 0).sum() >= 9
    rel = np.abs(got - want)[size > 0] / size[size > 0]
    print(f"sRGB gradient, {case}, colour space {color_space}: largest difference relative to the magnitudes deposited {rel.max():.3e} (bar 1e-6)")
    assert rel.max() <= 1e-6 and (got[size == 0] == 0).all()


def test_4096_rays_on_four_images(ctx, net):
    """4096 rays in their input order on four images in runs of 1024 (several workgroups, every wave on one image): the cells are exactly the integer sum of the
    per-ray deposits."""
    from nerfshop_amd import _abi, runtime
    n = 4096
    b = make_batch(seed=77, n_rays=n, max_count=3, live=n, clip=0, loss_type=rl.RELATIVE_L2, lin=True)
    b["ray_indices"] = np.arange(n, dtype=np.int32)
    u = upload(b)
    exp = runtime.Exposure(ctx, 4)
    values = exposures_for(4)
    exp.set(values)
    img = (np.arange(n) // 1024).astype(np.int32)
    pixels = t(np.stack([img, np.arange(n, dtype=np.int32)], 1), torch.int32)
    target, scale = exp.targets(u.ray_indices, u.counter, pixels, u.target)
    aux = torch.zeros((n, 12), dtype=torch.int32, device=DEV)
    outs = net.ray_loss(None, loss_params(b), u.numsteps, u.coords, u.out16, target, background=u.bg, ray_counter=u.counter, out=loss_buffers(b), aux=aux)
    acc = _abi.ExposureAccumulateParams(b["p"]["loss_scale"], 1)
    exp.accumulate(acc, u.counter, u.ray_indices, outs[0], aux, scale, n_rays=n)
    got = as_ints(exp.get(_abi.EXPOSURE_CELLS))
    want = ref.accumulate_cells(n, 4, n, b["ray_indices"], outs[0].cpu().numpy(), envmap_ref.split_aux(aux.cpu().numpy()), scale.cpu().numpy(), None, b["p"]["loss_scale"], True)
    assert got == want and all(got) and (outs[0].cpu().numpy()[:, 0] > 0).sum() >= 2000


# ---- step ---------------------------------------------------------------------------------------------------------------------------------------------------------
def read_state(exp):
    from nerfshop_amd import _abi
    return [exp.get(w) for w in (_abi.EXPOSURE_CELLS, _abi.EXPOSURE_VALUES, _abi.EXPOSURE_M, _abi.EXPOSURE_V)] + [exp.step_count()]


@pytest.mark.parametrize("n_images,l2_reg", [(1, 0.0), (5, 0.0), (70, 0.1), (1025, 0.0), (2500, 0.1)])
def test_step_is_the_host_twin(ctx, net, n_images, l2_reg):
    """Three accumulate + step rounds on one handle, from set values: after each, values, m and v are bit-equal to nrs_exposure_step_host on the state downloaded
    before it, within test_gpu_optimizer's bar of the float64 twin, and the cells are zero.  1025 and 2500 images: more than the step's 1024 threads (only a few of
    them have rays: the others move by momentum and the renormalisation)."""
    from nerfshop_amd import _abi, runtime
    b = make_batch(loss_type=rl.L2, lin=True, clip=CLIP)
    params = _abi.ExposureParams(l2_reg=l2_reg)
    exp = runtime.Exposure(ctx, n_images, params)
    exp.set(np.random.default_rng(n_images).uniform(-1.0, 1.0, (n_images, 3)).astype(f32))
    u = upload(b)
    img = (np.arange(R) * 13 % n_images).astype(np.int32)
    pixels = t(np.stack([img, np.arange(R, dtype=np.int32)], 1), torch.int32)
    aux = torch.zeros((R, 12), dtype=torch.int32, device=DEV)
    acc = _abi.ExposureAccumulateParams(b["p"]["loss_scale"], 1)
    loss_scale = float(b["p"]["loss_scale"])
    for k, lr in enumerate((1e-2, 3e-3, 1e-2)):
        target, scale = exp.targets(u.ray_indices, u.counter, pixels, u.target)
        outs = net.ray_loss(None, loss_params(b), u.numsteps, u.coords, u.out16, target, background=u.bg, ray_counter=u.counter, out=loss_buffers(b), aux=aux)
        exp.accumulate(acc, u.counter, u.ray_indices, outs[0], aux, scale, n_rays=R)
        before = read_state(exp)
        assert before[0].any() and before[4] == k
        exp.step(loss_scale=loss_scale, lr=lr)
        after = read_state(exp)
        assert not after[0].any() and after[4] == k + 1 and not exp.get(_abi.EXPOSURE_GRADIENT).any(), "the cells are zero afterwards"
        host = runtime.exposure_step_host(*before, loss_scale, lr, params=params)
        t64 = ref.step(*before, loss_scale, lr, l2_reg=l2_reg, dtype=np.float64)
        for j, name in ((2, "m"), (3, "v")):
            e_gpu = float(optimizer_ref.ulp_error(after[j], t64[j]).max())
            e_32 = float(optimizer_ref.ulp_error(host[j], t64[j]).max())
            assert e_gpu <= 4.0 * e_32 + 1.0, (name, e_gpu, e_32)
        size = np.spacing(f32(2.0 * np.abs(t64[1]).max()))
        e_gpu, e_32 = (float((np.abs(x.astype(np.float64) - t64[1]) / size).max()) for x in (after[1], host[1]))
        assert e_gpu <= 4.0 * e_32 + 1.0, ("values", e_gpu, e_32)
        for j, name in ((1, "values"), (2, "m"), (3, "v")):
            assert after[j].tobytes() == host[j].tobytes(), f"step {k}: {name} is bit-equal to the host twin"
        no_rays = ~before[0].any(axis=1)
        if n_images > 1 and no_rays.any():
            assert (after[1] != before[1])[no_rays].any(), "an image without rays still moves"
        total = np.abs(after[1].astype(np.float64).sum(axis=0))
        assert (total <= n_images * np.spacing(f32(np.abs(after[1]).max()))).all(), "zero mean per channel"
