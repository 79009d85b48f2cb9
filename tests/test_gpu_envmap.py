"""The trainable environment map on the GPU against tests/envmap_ref.py: nrs_envmap_background, nrs_ray_loss_ex, nrs_envmap_accumulate, nrs_envmap_step.

One batch for everything, the smallest that can still go wrong: 200 ray slots (not a multiple of 64 or 256) of 0..130 samples (ray_loss_ref.random_batch: rays the
opaque samples stop, M < n, rays of more than 64 samples, rays without samples), 187 of them below the counter, a compact buffer 37 samples short of what they
consume (the last rays are clipped), slots in a permuted order of the rays, and directions at both poles, on both sides of the phi = +-pi seam (tx + 1 wraps) and
anywhere else; maps of 1 x 1, 2 x 1, 5 x 3 and 8 x 4.

Bars.  Footprint: tx + wx against the float64 lookup within 1e-6 (res - 1), the angle error tests/test_gpu_modes.py states for this lookup (acosf / atan2f: 1e-6 in
the angle) times res - 1; the sum is compared, not its parts (a weight near 1 may flip to the next texel).  background_linear: against the float64 lookup under
test_gpu_modes' frame bar for an envmap (6e-3), and against the twin's float32 lookup AT THE DEVICE'S FOOTPRINT within 1e-5 relative (test_gpu_ray_loss' bar for a
per-ray quantity; texels and backgrounds are non-negative here, nothing cancels).  The aux record: n and M exact; C and target within 2^-20 (|C| + |target|) per
channel (test_gpu_ray_loss' allowance for the float32 error of C); T relative 2^-23 (1.5 M + 40) -- per factor one rounding of the product and one float32 step of
__expf, 1.5 x 2^-23, and the argument's two roundings carried through the exponential, 2 x 2^-24 per unit of optical depth, of which a ray holds at most
-ln(1e-4) = 9.2 before its last sample and 30 in it; g against loss_and_gradient in float64 ON THE DEVICE'S (target, C) within 1e-6 relative (four float32
roundings).  Rays whose transmittance comes within a relative 1e-3 of the stop threshold are left out, as in test_gpu_ray_loss.
The cells are compared bit for bit wherever no powf is involved; the sRGB bar is stated at its test."""
import ctypes as C

import numpy as np
import pytest
import torch

import envmap_ref as ref
import optimizer_ref
import ray_loss_ref as rl

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
MAPS = [(1, 1), (2, 1), (5, 3), (8, 4)]
R, LIVE = 200, 187


@pytest.fixture(scope="module")
def ctx(built):
    from nerfshop_amd import runtime
    return runtime.Context(0)


@pytest.fixture(scope="module")
def net(ctx):
    """a model that carries the two activations and the unit box (the ray loss reads nothing else of it)"""
    from nerfshop_amd import runtime, synth
    desc = synth.model_desc(1, log2_hashmap_size=14)
    desc.rgb_activation, desc.density_activation = rl.ACT_LOGISTIC, rl.ACT_EXPONENTIAL
    return runtime.NerfNetwork(ctx, desc, cell_cache_bytes=0)


def directions(rng, n):
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[0], d[1] = (0, 1, 0), (0, -1, 0)                                    # the poles: theta = 0 and pi
    d[2], d[3] = (-1e-4, 0.0, -1.0), (1e-4, 0.0, -1.0)                    # phi = +pi - 1e-4 and -pi + 1e-4
    d[4], d[5] = (-1e-4, 0.3, -1.0), (1e-4, -0.7, -1.0)
    d[6], d[7] = (0.0, 0.0, -1.0), (-0.0, 0.0, -1.0)                      # phi = atan2(-0, -1) = -pi and atan2(+0, -1) = +pi: the seam itself
    d[2:8] /= np.linalg.norm(d[2:8], axis=1, keepdims=True)
    return d.astype(f32)


def make_batch(seed=61, n_rays=R, max_count=130, live=LIVE, clip=37, **params):
    """the batch of the module docstring as a dict: ray_loss_ref's batch + rays [n, 6], ray_indices [n] (a permutation), live, cap"""
    b = rl.random_batch(seed, n_rays=n_rays, max_count=max_count, **params)
    rng = np.random.default_rng(seed + 1)
    b["numsteps"][[10, n_rays // 2], 0] = 0   # two rays without samples (their records stay where they are: a gap)
    b["rays"] = np.concatenate([rng.random((n_rays, 3)).astype(f32), directions(rng, n_rays)], 1)
    idx = rng.permutation(n_rays).astype(np.int32)
    for k in range(8):   # the poles and the seam sit in the first eight slots: live under every counter
        j = int(np.nonzero(idx == k)[0][0])
        idx[j], idx[k] = idx[k], k
    b["ray_indices"] = idx
    b["live"] = live
    if clip:
        b["p"]["cap"] = rl.closed_form(b).counter - clip
    return b


def texels_for(res_x, res_y, seed=5):
    return np.random.default_rng(seed + 10 * res_x + res_y).random((res_y, res_x, 4)).astype(f32)


def t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


class Run:
    pass


def upload(b):
    n = b["out"].shape[0]
    full = np.zeros((n, 16), np.float16)
    full[:, :4] = b["out"].astype(np.float16)
    u = Run()
    u.out16, u.numsteps, u.coords = t(full, torch.float16), t(b["numsteps"], torch.int32), t(b["coords"], torch.float32)
    u.target, u.bg = t(b["target"], torch.float32), None if b["background"] is None else t(b["background"], torch.float32)
    u.rays, u.ray_indices = t(b["rays"], torch.float32), t(b["ray_indices"], torch.int32)
    u.counter = torch.tensor([b["live"]], dtype=torch.int32, device=DEV)
    return u


def loss_params(b):
    from nerfshop_amd import _abi
    p = b["p"]
    return _abi.RayLossParams(loss_type=p["loss_type"], loss_scale=p["loss_scale"], color_space=p["color_space"], train_in_linear_colors=int(p["lin"]),
                              background=p["background"], near_distance=p["near_distance"], density_l1_reg=int(p["l1"]), max_samples_compacted=p["cap"])


def loss_buffers(b):
    n_rays, cap, ld = b["numsteps"].shape[0], b["p"]["cap"], b["coords"].shape[1]
    nan = float("nan")
    return (torch.full((n_rays, 2), -1, dtype=torch.int32, device=DEV), torch.full((cap, ld), nan, dtype=torch.float32, device=DEV),
            torch.full((cap, 16), nan, dtype=torch.float16, device=DEV), torch.full((n_rays,), nan, dtype=torch.float32, device=DEV),
            torch.full((1,), -1, dtype=torch.int32, device=DEV))


def pipeline(ctx, net, b, res, envmap_loss_type=None, texels="random", u=None, accumulate=True):
    """background -> ray_loss(background_linear, aux) -> accumulate on a fresh envmap of resolution `res`; everything the checks need, on the host"""
    from nerfshop_amd import _abi, runtime
    u = upload(b) if u is None else u
    env = runtime.Envmap(ctx, *res)
    tex = texels_for(*res) if isinstance(texels, str) else texels
    if tex is not None:
        env.set_texels(tex)
    n_rays = b["numsteps"].shape[0]
    bg_linear = torch.full((n_rays, 3), float("nan"), dtype=torch.float32, device=DEV)
    footprint = torch.full((n_rays, 4), -7, dtype=torch.int32, device=DEV)
    aux = torch.full((n_rays, 12), -7, dtype=torch.int32, device=DEV)
    env.background(u.rays, u.ray_indices, u.counter, background=u.bg, default_background=b["p"]["background"], out=(bg_linear, footprint))
    outs = net.ray_loss(None, loss_params(b), u.numsteps, u.coords, u.out16, u.target, background=u.bg, ray_counter=u.counter, out=loss_buffers(b),
                        background_linear=bg_linear, aux=aux)
    p = b["p"]
    r = Run()
    r.env, r.u, r.tex = env, u, tex
    r.acc = _abi.EnvmapAccumulateParams(p["loss_type"], p["loss_type"] if envmap_loss_type is None else envmap_loss_type, p["loss_scale"], int(p["lin"]))
    r.d = (bg_linear, footprint, aux, outs[0])
    if accumulate:
        env.accumulate(r.acc, u.counter, outs[0], aux, bg_linear, footprint, n_rays=n_rays)
    torch.cuda.synchronize()
    r.bg_linear, r.footprint, r.aux_words, r.numsteps_out = bg_linear.cpu().numpy(), footprint.cpu().numpy(), aux.cpu().numpy(), outs[0].cpu().numpy()
    r.outs = [x.cpu().numpy() for x in outs]
    r.aux = ref.split_aux(r.aux_words)
    r.cells = env.get(_abi.ENVMAP_CELLS) if accumulate else None
    return r


def want_cells(b, r, res, cells=None):
    return ref.accumulate_cells(res[0], res[1], b["numsteps"].shape[0], b["live"], r.numsteps_out, r.aux, r.bg_linear, r.footprint, r.acc.loss_type,
                                r.acc.envmap_loss_type, b["p"]["loss_scale"], bool(b["p"]["lin"]), cells=cells)


def as_ints(cells):
    return [int(c) for c in np.asarray(cells).reshape(-1)]


@pytest.fixture(scope="module")
def batch():
    b = make_batch()
    f = rl.closed_form(b).f
    n, M, live = f.N.numpy(), f.M.numpy(), np.arange(R) < LIVE
    Mc = rl.closed_form(b).numsteps_out.numpy()[:, 0]
    assert ((M < n) & live).sum() >= 5, "rays the opaque samples stop"
    assert ((n > 64) & (M == n) & live).sum() >= 5, "rays of more than 64 samples that reach the background"
    assert ((Mc < M) & live).sum() >= 1, "rays the compact buffer clips"
    assert ((n == 0) & live).sum() >= 1 and ((Mc == n) & (n > 0) & live).sum() >= 50
    return b


# ---- equivalence ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_ray_loss_ex_without_additions_is_ray_loss(ctx, net, batch):
    """nrs_ray_loss_ex with both new pointers NULL writes nrs_ray_loss's bits into every output; with the aux record alone the five old outputs are still bit-equal."""
    from nerfshop_amd.runtime._base import _stream_handle
    b, u = batch, upload(batch)
    plain = net.ray_loss(None, loss_params(b), u.numsteps, u.coords, u.out16, u.target, background=u.bg, ray_counter=u.counter, out=loss_buffers(b))
    bufs = loss_buffers(b)
    p = loss_params(b)
    st = net.lib.nrs_ray_loss_ex(net.h, _stream_handle(None), C.byref(p), R, u.counter.data_ptr(), u.numsteps.data_ptr(), b["out"].shape[0], u.coords.data_ptr(), 7,
                                 u.out16.data_ptr(), 16, 1, u.target.data_ptr(), u.bg.data_ptr(), None, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), 16, 1,
                                 bufs[3].data_ptr(), bufs[4].data_ptr(), None, None)
    assert st == 0
    aux = torch.full((R, 12), -7, dtype=torch.int32, device=DEV)
    with_aux = net.ray_loss(None, loss_params(b), u.numsteps, u.coords, u.out16, u.target, background=u.bg, ray_counter=u.counter, out=loss_buffers(b), aux=aux)
    torch.cuda.synchronize()
    for x, y, z in zip(plain, bufs, with_aux):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() == z.cpu().numpy().tobytes()
    a = ref.split_aux(aux.cpu().numpy())
    assert (aux.cpu().numpy()[LIVE:] == -7).all(), "slots at or past the counter are not written"
    assert (a["n"][:LIVE] >= a["M"][:LIVE]).all() and (a["n"][:LIVE] == np.where(b["numsteps"][:LIVE, 0] <= 1024, b["numsteps"][:LIVE, 0], 0)).all()
    assert int(plain[4].cpu()[0]) == int(a["M"][:LIVE].sum()), "the counter is the sum of M"


# ---- background and aux ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", MAPS)
def test_background_footprint_and_aux(ctx, net, batch, res):
    b = batch
    r = pipeline(ctx, net, b, res, accumulate=False)
    slots = np.arange(R)
    live = slots < LIVE
    assert (r.footprint[~live] == -7).all() and np.isnan(r.bg_linear[~live]).all(), "slots at or past the counter are not written"
    dirs = b["rays"][b["ray_indices"], 3:]
    fx, fy = ref.footprint64(dirs, *res)
    tx, ty = r.footprint[:, 0].astype(np.float64), r.footprint[:, 1].astype(np.float64)
    w = r.footprint[:, 2:4].copy().view(f32).astype(np.float64)
    ex, ey = np.abs(tx + w[:, 0] - fx)[live], np.abs(ty + w[:, 1] - fy)[live]
    print(f"{res}: footprint error x {ex.max():.3e} (bar {1e-6 * (res[0] - 1):.1e}), y {ey.max():.3e} (bar {1e-6 * (res[1] - 1):.1e})")
    assert ex.max() <= 1e-6 * (res[0] - 1) and ey.max() <= 1e-6 * (res[1] - 1)
    assert ((w >= 0) & (w < 1))[live].all() and (r.footprint[live, 0] >= 0).all() and (r.footprint[live, 0] <= res[0] - 1).all()
    if res[0] > 1:  # the seam: both sides are there, and on the far side tx + 1 wraps
        assert (r.footprint[live, 0] == res[0] - 1).any() and (r.footprint[live, 0] == 0).any()
    bg_slot = b["background"]
    # (a) float32 arithmetic at the device's own footprint
    want32 = ref.background_linear(r.tex, r.footprint[:, 0], r.footprint[:, 1], w[:, 0].astype(f32), w[:, 1].astype(f32), bg_slot)
    rel = (np.abs(r.bg_linear.astype(np.float64) - want32) / np.abs(want32))[live]
    # (b) everything in float64 from the direction on
    tx64, ty64 = np.floor(fx), np.floor(fy)
    tex64 = r.tex.astype(np.float64)
    env64 = np.zeros((R, 4))
    for k in range(R):
        cs = ref.corners(tx64[k], ty64[k], *res)
        wx, wy = fx[k] - tx64[k], fy[k] - ty64[k]
        for (x, y), wk in zip(cs, ((1 - wx) * (1 - wy), wx * (1 - wy), (1 - wx) * wy, wx * wy)):
            env64[k] += wk * tex64[y, x]
    lin = rl.srgb_to_linear(torch.as_tensor(bg_slot.astype(np.float64))).numpy()
    want64 = env64[:, :3] + lin * (1.0 - env64[:, 3:4])
    err64 = np.abs(r.bg_linear - want64)[live]
    print(f"{res}: background_linear against the float32 twin at the device's footprint {rel.max():.3e} relative (bar 1e-5); against float64 {err64.max():.3e} (bar 6e-3)")
    assert rel.max() <= 1e-5 and err64.max() <= 6e-3
    # the aux record
    a64 = ref.aux_record(b, r.bg_linear)
    keep = live & ~a64["near_threshold"]
    assert keep.sum() >= 0.99 * LIVE
    assert (r.aux["n"][keep] == a64["n"][keep]).all() and (r.aux["M"][keep] == a64["M"][keep]).all()
    M = a64["M"].astype(np.float64)
    reached = keep & (a64["M"] == a64["n"])   # T behind the LAST sample: of a ray the samples did not stop (no other T is read by anything)
    eT = (np.abs(r.aux["T"] - a64["T"]) / a64["T"])[reached]
    barT = (2.0 ** -23 * (1.5 * M + 40))[reached]
    size = np.abs(a64["C"]) + np.abs(a64["target"])
    eC, eTg = (np.abs(r.aux["C"] - a64["C"]) / size)[keep], (np.abs(r.aux["target"] - a64["target"]) / size)[keep]
    p = b["p"]
    _, g_dev = rl.loss_and_gradient(p["loss_type"], torch.as_tensor(r.aux["target"].astype(np.float64)), torch.as_tensor(r.aux["C"].astype(np.float64)))
    eg = (np.abs(r.aux["g"] - g_dev.numpy()) / np.maximum(np.abs(g_dev.numpy()), 1e-30))[keep]
    print(f"{res}: aux T {float((eT / barT).max()):.3f} of its bar, C {eC.max() * 2 ** 20:.3f} and target {eTg.max() * 2 ** 20:.3f} x 2^-20 (|C| + |target|), g {eg.max():.3e} relative")
    assert (eT <= barT).all() and eC.max() <= 2.0 ** -20 and eTg.max() <= 2.0 ** -20 and eg.max() <= 1e-6


# ---- accumulate, exact --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", MAPS)
@pytest.mark.parametrize("losses", [(rl.L2, None), (rl.RELATIVE_L2, None), (rl.L2, rl.RELATIVE_L2), (rl.HUBER, rl.L2)])
def test_accumulate_cells_are_exact(ctx, net, res, losses):
    """train_in_linear_colors: no powf between the record and the cells, so the cells are the twin's integers bit for bit, computed from the device's own footprint,
    aux record, numsteps_out and background_linear.  (step loss, envmap loss): the same, and differing -- the gradient recomputed from (target, C)."""
    b = make_batch(loss_type=losses[0], lin=True)
    r = pipeline(ctx, net, b, res, envmap_loss_type=losses[1])
    want = want_cells(b, r, res)
    got = as_ints(r.cells)
    assert got == want
    ok = ref.deposits(r.aux, r.numsteps_out, LIVE)
    stopped = (np.arange(R) < LIVE) & (r.aux["M"] < r.aux["n"])
    clipped = (np.arange(R) < LIVE) & (r.numsteps_out[:, 0] < r.aux["M"])
    assert ok.sum() >= 50 and stopped.sum() >= 5 and clipped.sum() >= 1 and not (ok & (stopped | clipped)).any()
    assert sum(1 for c in got if c) >= min(3 * res[0] * res[1], 12), "the gradient is there"
    assert all(c == 0 for c in got[3::4]), "alpha cells are zero"
    # nothing but the depositing slots reaches the cells: the same call on the records of those slots alone (the others' counts zeroed) gives the same cells
    from nerfshop_amd import _abi, runtime
    env2 = runtime.Envmap(ctx, *res)
    ns = r.d[3].clone()
    ns[torch.from_numpy(~ok).to(DEV), 0] = -1
    env2.accumulate(r.acc, r.u.counter, ns, r.d[2], r.d[0], r.d[1], n_rays=R)
    assert as_ints(env2.get(_abi.ENVMAP_CELLS)) == got


# ---- accumulate, sRGB ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("color_space", [rl.LINEAR, rl.SRGB])
def test_accumulate_srgb_gradient(ctx, net, color_space):
    """Without train_in_linear_colors the divisor srgb_to_linear_derivative(linear_to_srgb(background)) contains two powf.  The float gradient is compared with the
    float64 evaluation of the same expressions on the device's record, per cell relative to the sum of the magnitudes deposited there (deposits of both signs meet
    in a cell).  Measured on an MI355X (profiles/envmap_training.md): 2.6e-7 at worst (2.59e-7 in the Linear colour space, 2.51e-7 in sRGB).  The bar is 1e-6,
    just under 4 x that: the device library's powf is within 2 ulp where the measurement happened to see less, and the two powers carry their error into the
    quotient with exponents 0.41666 and 1.4."""
    from nerfshop_amd import _abi
    res = (8, 4)
    b = make_batch(loss_type=rl.L2, color_space=color_space, lin=False)
    r = pipeline(ctx, net, b, res, envmap_loss_type=rl.RELATIVE_L2)
    got = r.env.get(_abi.ENVMAP_GRADIENT).reshape(-1).astype(np.float64)
    assert (got == ref.cells_to_gradient(as_ints(r.cells)).astype(np.float64)).all(), "the gradient is the cells' own expression"
    a = r.aux
    ok = ref.deposits(a, r.numsteps_out, LIVE)
    tg, Cc = a["target"].astype(np.float64), a["C"].astype(np.float64)
    lg = 2.0 * (Cc - tg) / (Cc * Cc + 1e-2)
    bgl = r.bg_linear.astype(np.float64)
    srgb = np.where(bgl < 0.0031308, 12.92 * bgl, 1.055 * np.power(np.maximum(bgl, 0.0031308), float(f32(0.41666))) - 0.055)
    deriv = np.where(srgb <= 0.04045, 1.0 / 12.92, 2.4 / 1.055 * np.power((np.maximum(srgb, 0.04045) + 0.055) / 1.055, 1.4))
    v = (float(f32(b["p"]["loss_scale"])) / R) * (a["T"].astype(np.float64)[:, None] * lg) / deriv
    w = r.footprint[:, 2:4].copy().view(f32).astype(np.float64)
    want, size = np.zeros(4 * res[0] * res[1]), np.zeros(4 * res[0] * res[1])
    for s in np.nonzero(ok)[0]:
        wx, wy = w[s]
        for (x, y), wk in zip(ref.corners(r.footprint[s, 0], r.footprint[s, 1], *res), ((1 - wx) * (1 - wy), wx * (1 - wy), (1 - wx) * wy, wx * wy)):
            for c in range(3):
                want[4 * (x + y * res[0]) + c] += v[s, c] * wk
                size[4 * (x + y * res[0]) + c] += abs(v[s, c] * wk)
    assert (np.abs(v[ok]) < 512).all() and (size[0::4] > 0).all()
    rel = np.abs(got - want)[size > 0] / size[size > 0]
    print(f"sRGB gradient, colour space {color_space}: largest difference relative to the magnitudes deposited {rel.max():.3e} (bar 1e-6)")
    assert rel.max() <= 1e-6 and (got[3::4] == 0).all()


# ---- order --------------------------------------------------------------------------------------------------------------------------------------------------------
def test_cells_do_not_depend_on_the_order(ctx, net):
    """The same rays in a permuted slot order give bit-identical cells, and so do two calls (a float-atomic implementation fails the first).  Nothing is clipped here:
    which ray the compact buffer clips depends on the order by definition."""
    res = (5, 3)
    b = make_batch(loss_type=rl.L2, lin=True, live=R, clip=0)
    first = pipeline(ctx, net, b, res)
    again = pipeline(ctx, net, b, res)
    assert as_ints(first.cells) == as_ints(again.cells) == want_cells(b, first, res)
    perm = np.random.default_rng(3).permutation(R)
    b2 = dict(b, numsteps=b["numsteps"][perm], target=b["target"][perm], background=b["background"][perm], ray_indices=b["ray_indices"][perm])
    shuffled = pipeline(ctx, net, b2, res)
    assert (shuffled.aux_words == first.aux_words[perm]).all(), "a slot's record does not depend on where the slot is"
    assert as_ints(shuffled.cells) == as_ints(first.cells)
    assert sum(1 for c in as_ints(first.cells) if c) == 3 * 5 * 3


def test_4096_rays_into_one_footprint(ctx, net):
    """4096 rays of one direction (several workgroups, every deposit on the same four texels): the cells are exactly the integer sum of the per-ray deposits."""
    res = (8, 4)
    b = make_batch(seed=77, n_rays=4096, max_count=3, live=4096, clip=0, loss_type=rl.RELATIVE_L2, lin=True)
    b["rays"][:, 3:] = np.asarray([0.48, 0.6, 0.64], f32)
    r = pipeline(ctx, net, b, res)
    assert (r.footprint == r.footprint[0]).all()
    got = as_ints(r.cells)
    assert got == want_cells(b, r, res)
    assert sum(1 for c in got if c) == 12 and ref.deposits(r.aux, r.numsteps_out, 4096).sum() >= 2000


# ---- step ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_first_step_from_zero_texels(ctx, net):
    """A fresh envmap is all zeros.  After accumulate and the first step every texel channel whose gradient is non-zero holds the optimiser's rule on that gradient
    (optimizer_ref: judged like tests/test_gpu_optimizer.py, against twin64 within 4 x twin32's error + 1 float32 step), which from zero moments is -lr * sign(g) to
    within epsilon / (0.1 |g|); every other channel and every alpha is bit-equal to before; the cells are zero again; the EMA follows the rule (a = 0, b = 1 at the
    first step: the fp16 copy of the texels)."""
    from nerfshop_amd import _abi
    res, lr, loss_scale = (8, 4), 1e-2, 128.0
    b = make_batch(loss_type=rl.L2, lin=True)
    r = pipeline(ctx, net, b, res, envmap_loss_type=rl.RELATIVE_L2, texels=None)
    env = r.env
    assert (env.get(_abi.ENVMAP_TEXELS) == 0).all() and (env.get(_abi.ENVMAP_EMA) == 0).all(), "a fresh map is all zeros"
    cells = as_ints(r.cells)
    assert cells == want_cells(b, r, res)
    grad = ref.cells_to_gradient(cells)
    assert (env.get(_abi.ENVMAP_GRADIENT).reshape(-1) == grad).all()
    env.step(loss_scale=loss_scale, lr=lr)
    texels, ema = env.get(_abi.ENVMAP_TEXELS).reshape(-1), env.get(_abi.ENVMAP_EMA).reshape(-1)
    assert not any(as_ints(env.get(_abi.ENVMAP_CELLS))) and (env.get(_abi.ENVMAP_GRADIENT) == 0).all(), "the cells are all zero again"
    assert env.step_count() == 1
    st = ref.fresh_state(np.zeros(grad.size, f32))
    t64, t32 = ref.step(st, grad, loss_scale, lr), ref.step(st, grad, loss_scale, lr, twin=optimizer_ref.twin32)
    moved = grad != 0
    assert moved.sum() >= 40 and not moved[3::4].any()
    assert (texels[~moved].view(np.uint32) == 0).all(), "zero gradient and alpha: bit-equal to before"
    e_gpu = float(optimizer_ref.ulp_error(texels[moved], t64.master[moved]).max())
    e_32 = float(optimizer_ref.ulp_error(t32.master[moved], t64.master[moved]).max())
    print(f"first step: texels {e_gpu:.2f} float32 steps from twin64 (twin32: {e_32:.2f}); bit-equal to twin32: {bool((texels == t32.master).all())}")
    assert e_gpu <= 4.0 * e_32 + 1.0
    big = moved & (np.abs(grad / f32(loss_scale)) >= 1e-4)
    assert big.sum() >= 20 and np.abs(texels[big] + lr * np.sign(grad[big])).max() <= lr * 2e-5, "-lr * sign(g): epsilon / (0.1 |g|) <= 1e-5 here"
    want_ema = ref.step(st, grad, loss_scale, lr, fp16_for_ema=texels.astype(np.float16)).ema
    assert optimizer_ref.ulp_error(ema, want_ema).max() <= 1.0 and (ema == texels.astype(np.float16).astype(f32)).all()
    # export: the live and the EMA texels as a tensor, what Testbed.envmap takes
    assert (env.export(ema=False).cpu().numpy().reshape(-1) == texels).all() and (env.export(ema=True).cpu().numpy().reshape(-1) == ema).all()
    # set_texels resets the optimiser: the EMA becomes the texels, the step count 0
    env.set_texels(texels_for(*res))
    assert (env.get(_abi.ENVMAP_EMA) == texels_for(*res)).all() and env.step_count() == 0
