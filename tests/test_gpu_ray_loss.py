"""nrs_training_samples and nrs_ray_loss on the GPU against the twins of tests/ray_loss_ref.py, and the torch surface on top of them.

dL/doutput is always judged in the accuracy unit of ray_loss_ref.error_units (what is left of |got - exact| after 2^-11 of the value, the rounding of the stored
fp16, in float32 steps of the sizes of the terms that form the element), against closed_form (float64).  The bar is 4 x the worst error of closed_form32 -- the
reference's own float32 arithmetic, its result stored as fp16 like the kernel's -- on the same inputs.  A ray is left out of a comparison iff the twin sees a
transmittance within a relative 1e-3 of the stop threshold.

Measured (MI355X; every case is in profiles/ray_loss.md): over all elements the kernel meets the bar in all 42 cases that compare a gradient, but in 35 of them
both sides are 8 384 512 = 2^23 (1 - 2^-11): an element whose only term is below half of fp16's smallest step is stored as 0 and scores 2^23 whoever computes it,
and the measure, kept as the issue states it, has no allowance for that step -- so that assertion alone could not fail.  judge() therefore also asserts the same
unit and factor over the elements whose exact value is a normal fp16 (|v| >= 2^-14); there the kernel scores between 0 and 3534 units (8097 before it summed a
sample's suffix from the ray's far end, profiles/training_large_scenes.md), closed_form32 between 0 and 9072.

"A cone's steps in a big box" (below) runs the loss where real captures train: dt up to 128 minimum steps (warped dt up to 8.47), the model's box of side 16 or 4,
the near-distance term against origins inside that box; the batches are pinned on the CPU by tests/test_ray_loss_host.py.  The generator and the Trainer in large
boxes are in tests/test_gpu_training_large_scenes.py; the figures of all of it in profiles/training_large_scenes.md."""
import ctypes as C

import numpy as np
import pytest
import torch

import ray_loss_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ctx(built):
    from nerfshop_amd import runtime
    return runtime.Context(0)


_NETS = {}


def network(ctx, rgb_act=ref.ACT_LOGISTIC, den_act=ref.ACT_EXPONENTIAL, aabb_scale=1):
    """a model that carries the two activations and the box of side aabb_scale (nrs_ray_loss reads nothing else of it)"""
    from nerfshop_amd import runtime, synth
    if (rgb_act, den_act, aabb_scale) not in _NETS:
        desc = synth.model_desc(aabb_scale, log2_hashmap_size=14)
        desc.rgb_activation, desc.density_activation = rgb_act, den_act
        _NETS[(rgb_act, den_act, aabb_scale)] = runtime.NerfNetwork(ctx, desc, cell_cache_bytes=0)
    return _NETS[(rgb_act, den_act, aabb_scale)]


def gpu_params(b):
    from nerfshop_amd import _abi
    p = b["p"]
    return _abi.RayLossParams(loss_type=p["loss_type"], loss_scale=p["loss_scale"], color_space=p["color_space"], train_in_linear_colors=int(p["lin"]),
                              background=p["background"], near_distance=p["near_distance"], density_l1_reg=int(p["l1"]), max_samples_compacted=p["cap"])


def run(ctx, b, planes_in=False, planes_out=False, live=None):
    """the batch through NerfNetwork.ray_loss with NaN-prefilled outputs; numpy results"""
    aabb_scale = int(b["aabb"][1][0] - b["aabb"][0][0])
    assert b["aabb"] == ref.scene_aabb(aabb_scale), "the model carries the box the batch names"
    net = network(ctx, b["rgb_act"], b["den_act"], aabb_scale)
    n, R, cap, ld = b["out"].shape[0], b["numsteps"].shape[0], b["p"]["cap"], b["coords"].shape[1]
    rng = np.random.default_rng(1)
    full = rng.normal(size=(n, 16)).astype(np.float16)  # rows 4..15: the rgb network's padding outputs, never read
    full[:, :4] = b["out"].astype(np.float16)
    assert (full[:, :4].astype(np.float64) == b["out"]).all(), "the batch's outputs must be fp16 values"
    if planes_in:
        out16 = torch.zeros((16, n + 5), dtype=torch.float16)
        out16[:, :n] = torch.from_numpy(full.T.copy())
    else:
        out16 = torch.from_numpy(full)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)
    nan = float("nan")
    bufs = (torch.full((R, 2), -1, dtype=torch.int32, device=DEV), torch.full((cap, ld), nan, dtype=torch.float32, device=DEV),
            torch.full((16, cap + 3) if planes_out else (cap, 16), nan, dtype=torch.float16, device=DEV), torch.full((R,), nan, dtype=torch.float32, device=DEV),
            torch.full((1,), -1, dtype=torch.int32, device=DEV))
    counter = None if live is None else torch.tensor([live], dtype=torch.int32, device=DEV)
    got = net.ray_loss(None, gpu_params(b), t(b["numsteps"], torch.int32), t(b["coords"], torch.float32), out16.to(DEV), t(b["target"], torch.float32),
                       background=None if b["background"] is None else t(b["background"], torch.float32),
                       ray_origins=None if b["origins"] is None else t(b["origins"], torch.float32), ray_counter=counter, out=bufs)
    torch.cuda.synchronize()
    numsteps_out, coords_out, dl, loss, count = (x.cpu().numpy() for x in got)
    dl = dl.T[:cap] if planes_out else dl
    return numsteps_out, coords_out, dl.astype(np.float64), loss, int(count[0])


def judge(name, b, got, exact_layout):
    """Compare one run with the twins; returns (worst GPU error, worst closed_form32 error, left-out share)."""
    numsteps_out, coords_out, dl, loss, count = got
    c, c32 = ref.closed_form(b), ref.closed_form32(b)
    f = c.f
    R, cap, live = f.R, b["p"]["cap"], f.live
    left_out = f.near_threshold.numpy().copy()
    if exact_layout:
        assert not left_out.any(), "a constructed batch has no transmittance near the threshold"
        assert count == c.counter
        assert (numsteps_out[:live] == c.numsteps_out.numpy()[:live]).all()
    assert (numsteps_out[live:] == -1).all(), "rays at or past the counter are not written"
    assert (loss[live:] == 0).all()
    want_M, want_dl, A, dl32 = c.numsteps_out.numpy()[:, 0], c.dl.numpy(), c.A.numpy(), c32.dl.numpy()
    same32 = (c32.f.M == f.M).numpy()
    worst_gpu = worst_32 = worst_gpu_n = worst_32_n = 0.0
    n_el = n_normal = beyond = 0
    beyond_by = 0.0
    end = 0
    for r in range(live):
        m, cb = int(numsteps_out[r, 0]), int(numsteps_out[r, 1])
        if not exact_layout:  # (these batches' compact buffers hold every sample: nothing is clipped, so a ray starts where the one before it ends)
            assert cb == end, (name, r)
            end = cb + m
        if left_out[r]:
            continue
        assert m == want_M[r], (name, r, m, int(want_M[r]))
        # 1e-5 relative; outside the constructed case a ray's colour may also lie within float32's reach of its target, where the loss (a function of C - target)
        # has no relative accuracy to speak of: there the float32 error of C itself is allowed for, 2^-20 (|C| + |target|) per channel -- sixteen float32 steps for
        # a sum of up to 130 terms -- carried into the loss by its derivative g
        slack = 0.0 if exact_layout else float((f.g[r].abs() * 2.0 ** -20 * (f.C[r].abs() + f.target[r].abs())).sum()) / 3.0 / float(b.get("n_rays", R))
        loss_err = abs(float(loss[r]) - float(c.loss[r]))
        if loss_err > 1e-5 * float(c.loss[r]):  # (reported: how many rays need the slack, and the largest miss as a multiple of 1e-5 relative)
            beyond += 1
            beyond_by = max(beyond_by, loss_err / (1e-5 * float(c.loss[r])))
        assert loss_err <= 1e-5 * float(c.loss[r]) + slack, (name, r, float(loss[r]), float(c.loss[r]))
        if m == 0:
            continue
        k0, src0 = int(c.numsteps_out[r, 1]), int(f.base[r])
        assert (coords_out[cb:cb + m].view(np.uint32) == b["coords"][src0:src0 + m].view(np.uint32)).all(), "compacted records are copies"
        e = ref.error_units(dl[cb:cb + m, :4], want_dl[k0:k0 + m], A[k0:k0 + m])
        worst_gpu = max(worst_gpu, float(e.max()))
        normal = np.abs(want_dl[k0:k0 + m]) >= 2.0 ** -14  # the exact value is a normal fp16: 2^-11 of it IS the stored value's rounding
        n_el, n_normal = n_el + normal.size, n_normal + int(normal.sum())
        worst_gpu_n = max(worst_gpu_n, float(np.where(normal, e, 0.0).max()))
        if same32[r]:
            e32 = ref.error_units(ref.to_fp16_values(dl32[k0:k0 + m]), want_dl[k0:k0 + m], A[k0:k0 + m])
            worst_32 = max(worst_32, float(e32.max()))
            worst_32_n = max(worst_32_n, float(np.where(normal, e32, 0.0).max()))
    tail = min(count, cap)
    assert (dl[tail:cap, :4] == 0).all() and (coords_out[tail:] == 0).all(), "the compact tail is zero"
    assert np.isnan(dl[:, 4:]).all(), "rows 4..15 are never written"
    share = float(left_out[:live].mean()) if live else 0.0
    print(f"{name}: dL/doutput worst error GPU {worst_gpu:.1f}, closed_form32 {worst_32:.1f} (units of 2^-23 A); left out {share * 100:.2f} % of {live} rays")
    print(f"{name}: fp16-normal elements ({n_normal} of {n_el}): GPU {worst_gpu_n:.1f}, closed_form32 {worst_32_n:.1f}; loss beyond 1e-5 relative: {beyond} rays, "
          f"worst {beyond_by:.2f} x 1e-5")
    # The issue's assertion stays with the callers.  Beside it, the same unit and the same factor over the elements whose exact value is a normal fp16 only: over all
    # elements both sides saturate at 2^23 on a gradient that underflows fp16 (an all-zero dL would pass); here a wrong sign, suffix or carry scores 10^6 and more.
    # In this range an element scores 0 unless its float32 error carries the value across an fp16 rounding boundary, and then it scores up to that float32 error;
    # closed_form32 has no such element at all in 5 of the 42 cases (a bar of 0).  So the bar has a floor, from the formats alone: a product of M factors and sums
    # of M terms carry up to M float32 half-steps each, M / 2 + M / 2 = M units for the longest ray consumed in the batch (130, or 1024 in the constructed case).
    floor = float(f.M.max())
    assert n_normal >= 0.3 * n_el
    assert worst_gpu_n <= 4.0 * max(worst_32_n, floor), (name, worst_gpu_n, worst_32_n, floor)
    return worst_gpu, worst_32, share


@pytest.mark.parametrize("planes_in,planes_out,ld", [(False, False, 7), (True, True, 8), (True, False, 7), (False, True, 8)])
def test_constructed_lengths(ctx, planes_in, planes_out, ld):
    """Counts either side of 32, 64, 128 and a 1024-sample ray, decisive stops at sample 0, mid-chunk, lanes 31|32, 63|64, N - 2 and N - 1; no ray is left out."""
    b, expect = ref.constructed_batch(3, ld=ld)
    f = ref.closed_form(b).f
    assert (f.M.numpy() == expect).all()
    assert not bool(f.in_band.any()), "no transmittance in front of a sample lies in [0.5e-4, 2e-4]"
    for stop in (1, 32, 33, 64, 65):
        assert ((expect == stop) & (f.N.numpy() > stop)).any(), stop
    assert ((expect == f.N.numpy() - 1) & (expect > 0)).any() and ((expect == f.N.numpy()) & (f.N.numpy() > 1)).any()
    got = run(ctx, b, planes_in, planes_out)
    worst_gpu, worst_32, share = judge(f"constructed (planes {planes_in}/{planes_out}, ld {ld})", b, got, True)
    assert share == 0.0
    assert worst_gpu <= 4.0 * worst_32


@pytest.mark.parametrize("loss_type", range(7))
@pytest.mark.parametrize("colour", [(ref.LINEAR, False), (ref.SRGB, False), (ref.SRGB, True)])
def test_every_loss_and_colour_path(ctx, loss_type, colour):
    """200 random rays of 0..130 samples, alpha of the target in {0, 0.5, 1}; per-ray background for even losses, the constant one for odd."""
    b = ref.random_batch(140 + loss_type, loss_type=loss_type, color_space=colour[0], lin=colour[1], per_ray_bg=loss_type % 2 == 0)
    worst_gpu, worst_32, share = judge(f"loss {loss_type} colour {colour}", b, run(ctx, b), False)
    assert share <= 0.01
    assert worst_gpu <= 4.0 * worst_32


@pytest.mark.parametrize("rgb_act", range(4))
@pytest.mark.parametrize("den_act", range(4))
def test_activations(ctx, rgb_act, den_act):
    """Every pair of activations, with the density regulariser and the near-distance term on.  Raw densities stay within the reach of each activation's step: a
    ReLU or plain density of up to 9 per unit length never stops a ray, the exponential one does."""
    b = ref.random_batch(70 + 4 * rgb_act + den_act, rgb_act_kind=rgb_act, den_act_kind=den_act, l1=True, near_distance=0.7, with_origins=True,
                         loss_type=ref.HUBER)
    worst_gpu, worst_32, share = judge(f"rgb activation {rgb_act} density activation {den_act}", b, run(ctx, b), False)
    assert share <= 0.01
    assert worst_gpu <= 4.0 * worst_32


# ---- a cone's steps in a big box ------------------------------------------------------------------------------------------------------------------------------------
def with_ld8(b):
    """the batch with records of 8 floats: the same samples, a padding float behind each"""
    pad = np.random.default_rng(5).random((b["coords"].shape[0], 1)).astype(np.float32)
    return dict(b, coords=np.ascontiguousarray(np.concatenate([b["coords"], pad], 1)))


@pytest.mark.parametrize("scale,planes", [(16, False), (4, False), (16, True)])
def test_long_steps_in_a_big_box(ctx, scale, planes):
    """ray_loss_ref.big_box_batch (pinned by tests/test_ray_loss_host.py): dt of 1..128 minimum steps -- warped dt up to 8.47, __expf(-density dt) at steps up to 100
    times longer than the other batches' -- in the box of side 16 and of side 4, Huber loss, the density regulariser, and the near-distance term, which unwarps every
    position through the model's box, against origins inside it.  Interleaved layouts; once more with plane layouts and records of 8 floats.  The bars are the other
    tests' bars.

    Measured on an MI355X (profiles/training_large_scenes.md), over the fp16-normal elements: GPU 0.0 in all three cases, closed_form32 231.4 (scale 16) and
    86.4 (scale 4).  This test found the gradient kernel forming what lies behind a sample as C - C2 AT the sample: at scale 4 that scored 778.4 against a bar of
    4 x max(86.4, 128) = 512, on the density gradient of sample 27 of a ray stopped after 30 (T rgb and the suffix both near 1e-3 of C, so half a float32 step of C
    was about 400 units).  The kernel now sums the later samples of the chunk from the ray's far end and takes C - C2 only there."""
    b = ref.big_box_batch(scale)
    if planes:
        b = with_ld8(b)
    worst_gpu, worst_32, share = judge(f"big box, scale {scale}, planes {planes}", b, run(ctx, b, planes, planes), False)
    assert share <= 0.01
    assert worst_gpu <= 4.0 * worst_32


@pytest.mark.parametrize("den_act", range(4))
def test_long_steps_with_every_density_activation(ctx, den_act):
    """The same long steps in the box of side 16 with each density activation, logistic colours.  Raw densities stay within the reach of each activation's step, as in
    test_activations: the exponential one's are lowered by ln(dt / MIN_STEP) (the builder does), so a sample's optical depth is what it is at short steps; a logistic
    density is below 1 per unit length, 0.22 per sample at the longest step; a plain or ReLU density per unit length is x - ln(steps) with x around 6 and at most 9,
    at most 0.9 per sample (at 128 steps, 4.15 x 0.2165), so that some rays stop and most do not, and few plain densities are negative."""
    mean = 3.0 if den_act in (ref.ACT_LOGISTIC, ref.ACT_EXPONENTIAL) else 6.0
    b = ref.big_box_batch(16, seed=350 + den_act, den_act_kind=den_act, density_mean=mean)
    worst_gpu, worst_32, share = judge(f"long steps, density activation {den_act}", b, run(ctx, b), False)
    assert share <= 0.01
    assert worst_gpu <= 4.0 * worst_32


def test_constructed_lengths_at_long_steps(ctx):
    """test_constructed_lengths with every dt at 64 minimum steps (warped 4.2) in the box of side 16: the densities derive from dt, so the stops stay decisive and the
    layout is exact."""
    b, expect = ref.constructed_batch(3, dt_steps=64.0)
    b["aabb"] = ref.scene_aabb(16)
    assert float(b["coords"][0, 3]) > 4.0
    f = ref.closed_form(b).f
    assert (f.M.numpy() == expect).all()
    assert not bool(f.in_band.any()), "no transmittance in front of a sample lies in [0.5e-4, 2e-4]"
    for stop in (1, 32, 33, 64, 65):
        assert ((expect == stop) & (f.N.numpy() > stop)).any(), stop
    assert ((expect == f.N.numpy() - 1) & (expect > 0)).any() and ((expect == f.N.numpy()) & (f.N.numpy() > 1)).any()
    worst_gpu, worst_32, share = judge("constructed, dt 64 steps", b, run(ctx, b), True)
    assert share == 0.0
    assert worst_gpu <= 4.0 * worst_32


def test_counter_cap_and_determinism(ctx):
    """Rays at or past the device counter do nothing; a compact buffer smaller than the sum of M clips the last rays (the counter stays unclipped); two calls agree bit for bit."""
    b = ref.random_batch(91, n_rays=120, max_count=80)
    total = ref.closed_form(b).counter
    b["live"] = 111
    live_total = ref.closed_form(b).counter
    assert live_total < total
    b["p"]["cap"] = live_total - 37
    c = ref.closed_form(b)
    assert int((c.numsteps_out[:111, 0] < c.f.M[:111]).sum()) >= 1 and c.counter == live_total
    first = run(ctx, b, live=111)
    judge("clipped", b, first, True)
    again = run(ctx, b, live=111)
    for x, y in zip(first[:4], again[:4]):
        assert x.tobytes() == y.tobytes()
    assert first[4] == again[4] == live_total


def test_loss_across_scan_tiles(ctx):
    """1079 rays: the scan of M takes two tiles of 1024 rays.  Whole; then with 1050 live rays and a compact buffer 37 samples short, which clips the last 37 rays,
    either side of the tile boundary; that run twice, bit for bit."""
    b, expect = ref.constructed_batch(3, repeats=13)
    c = ref.closed_form(b)
    assert b["numsteps"].shape[0] == 1079 and b["out"].shape[0] >= 27062 and c.counter == 14920
    assert (c.f.M.numpy() == expect).all() and not bool(c.f.in_band.any()) and not bool(c.f.near_threshold.any())
    judge("two tiles", b, run(ctx, b), True)
    b["live"] = 1050
    live_total = ref.closed_form(b).counter
    assert live_total == 14736
    b["p"]["cap"] = live_total - 37
    c = ref.closed_form(b)
    clipped = np.nonzero((c.numsteps_out[:1050, 0] < c.f.M[:1050]).numpy())[0]
    assert len(clipped) == 37 and clipped.min() < 1024 <= clipped.max() and c.counter == live_total   # (rays 1013..1049: either side of the tile boundary)
    first = run(ctx, b, live=1050)
    judge("two tiles, clipped", b, first, True)
    again = run(ctx, b, live=1050)
    for x, y in zip(first[:4], again[:4]):
        assert x.tobytes() == y.tobytes()
    assert first[4] == again[4] == live_total


def test_no_rays_and_refusals(ctx):
    from nerfshop_amd import _abi, runtime
    net = network(ctx)
    p = _abi.RayLossParams(max_samples_compacted=6)
    e = lambda *shape, dt=torch.float32: torch.full(shape, 7, dtype=dt, device=DEV)
    numsteps_out, coords_out, dl, loss, count = net.ray_loss(None, p, e(0, 2, dt=torch.int32), e(0, 7), e(0, 16, dt=torch.float16), e(0, 4),
                                                             out=(e(0, 2, dt=torch.int32), e(6, 7), e(6, 16, dt=torch.float16), e(0), e(1, dt=torch.int32)))
    torch.cuda.synchronize()
    assert int(count[0]) == 0 and float(coords_out.abs().max()) == 0 and float(dl[:, :4].abs().max()) == 0 and float(dl[:, 4:].min()) == 7
    with pytest.raises(runtime.NrsError):
        net.ray_loss(None, p, e(3, 2, dt=torch.int32), e(5, 6), e(5, 16, dt=torch.float16), e(3, 4))
    with pytest.raises(runtime.NrsError):
        net.ray_loss(None, p, e(3, 2, dt=torch.int32), e(5, 7), e(5, 16, dt=torch.float16), e(2, 4))
    rays = torch.zeros(4, 6, device=DEV)
    with pytest.raises(runtime.NrsError, match="occupancy"):  # NRS_ERR_STATE: no density bitfield yet
        net.training_samples(None, rays, None, 0.0, 16)
    from nerfshop_amd import synth
    lit = runtime.NerfNetwork(ctx, synth.model_desc(1, log2_hashmap_size=14), cell_cache_bytes=0, n_extra_dims=3)
    with pytest.raises(runtime.NrsError, match="n_extra_dims"):
        lit.training_samples(None, rays, None, 0.0, 16)
    lit.close()


# ---- the generator -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def generated(ctx, scene):
    """100 rays from outside the box (tests/test_ray_loss_host.py's), the twin's walk at three entry distances, and a model that holds the scene's occupancy"""
    from nerfshop_amd import runtime
    from oracle import oracle as orc
    rng = np.random.default_rng(21)
    o = rng.normal(size=(100, 3))
    o = (0.5 + 1.6 * o / np.linalg.norm(o, axis=1, keepdims=True)).astype(np.float32)
    d = rng.uniform(0.3, 0.7, (100, 3)).astype(np.float32) - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    rays, jitter = np.concatenate([o, d], 1).astype(np.float32), rng.random(100).astype(np.float32)
    lib = orc.load()
    walks = {k: ref.march(lib, scene.bitfield, ref.AABB_UNIT, rays, jitter, 0.0, tmin_nudge_ulps=k) for k in (-2, 0, 2)}
    counts = {k: np.array([len(r) for r in w]) for k, w in walks.items()}
    stable = (counts[-2] == counts[0]) & (counts[0] == counts[2])
    net = runtime.NerfNetwork(ctx, scene.desc, cell_cache_bytes=0)
    net.set_density_bitfield(scene.bitfield)
    return net, rays, jitter, walks[0], counts[0], stable


def test_training_samples_against_the_twin(generated):
    net, rays, jitter, walk, counts, stable = generated
    assert stable.mean() >= 0.98 and (counts > 0).sum() >= 30
    total = int(counts.sum())
    max_samples = total + 11
    coords, numsteps, ray_indices, counters = (x.cpu().numpy() for x in net.training_samples(None, torch.from_numpy(rays).to(DEV), torch.from_numpy(jitter).to(DEV), 0.0,
                                                                                              max_samples, ld=8))
    emitted = int(counters[0])
    got_counts = np.zeros(len(counts), np.int64)
    got_counts[ray_indices[:emitted]] = numsteps[:emitted, 0]
    assert (got_counts[stable] == counts[stable]).all(), "stable rays have the twin's sample count"
    # the layout is a function of the counts: the scan in input order, whatever the counts are
    want_numsteps, want_idx, want_counters, bases = ref.layout_from_counts(got_counts, max_samples)
    assert emitted == want_counters[0] and int(counters[1]) == want_counters[1]
    assert (ray_indices[:emitted] == want_idx).all() and (numsteps[:emitted] == want_numsteps).all()
    assert (numsteps[emitted:] == 0).all() and (ray_indices[emitted:] == 0).all()
    compared = 0
    for i in np.nonzero(stable & (counts > 0))[0]:
        rec = coords[bases[i]:bases[i] + counts[i], :7]
        assert (rec.view(np.uint32) == walk[i].view(np.uint32)).all(), f"ray {i}: records differ from the twin's"
        compared += len(rec)
    assert compared > 5000
    end = int(want_counters[1])
    assert (coords[end:, :7] == 0).all() and (coords[:, 7] == 0).all(), "zero tail; float 7 of a record is never written"


def test_training_samples_drops_clips_and_repeats(generated):
    """max_samples below the total: the ray that does not fit and every later one are dropped, the counter still counts them, the records behind the last emitted ray
    are zero; no jitter (NULL) and no rays are handled; two calls agree bit for bit."""
    net, rays, jitter, walk, counts, stable = generated
    d_rays = torch.from_numpy(rays).to(DEV)
    full = [x.cpu().numpy() for x in net.training_samples(None, d_rays, None, 0.0, 1 << 16)]
    got_counts = np.zeros(len(counts), np.int64)
    got_counts[full[2][:full[3][0]]] = full[1][:full[3][0], 0]
    cut = int(got_counts.sum()) * 2 // 3
    runs = [[x.cpu().numpy() for x in net.training_samples(None, d_rays, None, 0.0, cut)] for _ in range(2)]
    for x, y in zip(*runs):
        assert x.tobytes() == y.tobytes()
    coords, numsteps, ray_indices, counters = runs[0]
    want_numsteps, want_idx, want_counters, bases = ref.layout_from_counts(got_counts, cut)
    assert 0 < want_counters[0] < (got_counts > 0).sum()
    assert tuple(counters) == want_counters and (numsteps[:counters[0]] == want_numsteps).all() and (ray_indices[:counters[0]] == want_idx).all()
    end = int(want_numsteps[-1].sum())
    assert (coords[:end] == full[0][:end]).all() and (coords[end:] == 0).all()
    coords, numsteps, ray_indices, counters = net.training_samples(None, torch.zeros(0, 6, device=DEV), None, 0.0, 9)
    assert counters.tolist() == [0, 0] and float(coords.abs().max()) == 0
    # a ray the walk could not end on has no samples: zero direction, non-finite origin
    bad = rays[:4].copy()
    bad[0, 3:] = 0
    bad[1, 0] = np.inf
    bad[2, 3:] *= 1e-20
    c = net.training_samples(None, torch.from_numpy(bad).to(DEV), None, 0.0, 4096)[3].cpu().numpy()
    assert c[1] == got_counts[3] and c[0] == (1 if got_counts[3] else 0)


@pytest.fixture(scope="module")
def generated_100(generated):
    """the fixture's 100 rays through the generator once: per-ray counts and records"""
    net, rays, jitter, walk, counts, stable = generated
    coords, numsteps, ray_indices, counters = (x.cpu().numpy() for x in net.training_samples(None, torch.from_numpy(rays).to(DEV), torch.from_numpy(jitter).to(DEV), 0.0,
                                                                                              1 << 16))
    emitted = int(counters[0])
    assert int(counters[1]) <= 1 << 16 and emitted == (counts > 0).sum() > 30
    got_counts = np.zeros(100, np.int64)
    got_counts[ray_indices[:emitted]] = numsteps[:emitted, 0]
    records = [np.zeros((0, 7), np.float32)] * 100
    for k in range(emitted):
        records[ray_indices[k]] = coords[numsteps[k, 1]:numsteps[k, 1] + numsteps[k, 0]]
    return got_counts, records


@pytest.mark.parametrize("n,cut", [(1023, False), (1024, False), (1025, False), (2600, False), (2600, True)])
def test_training_samples_across_scan_tiles(generated, generated_100, n, cut):
    """The 100 rays repeated to n: one tile of 1024 rays less one ray, exactly one tile, one ray into the second, and three tiles; cut: max_samples drops a ray of the
    second tile and every ray behind it.  The layout is layout_from_counts of the 100-ray call's counts, a ray's records are those of the 100-ray call, byte for
    byte, the tail is zero, and two calls agree."""
    net, rays, jitter = generated[:3]
    counts100, records = generated_100
    which = np.arange(n) % 100
    counts = counts100[which]
    max_samples = int(counts.sum()) + 11
    if cut:
        bases = np.cumsum(counts) - counts
        k = 1500 + int(np.nonzero(counts[1500:])[0][0])
        max_samples = int(bases[k] + counts[k]) - 1   # ray k is the first that does not fit
        assert 1024 <= k < 2048
    d_rays, d_jitter = torch.from_numpy(rays[which]).to(DEV), torch.from_numpy(jitter[which]).to(DEV)
    runs = [[x.cpu().numpy() for x in net.training_samples(None, d_rays, d_jitter, 0.0, max_samples)] for _ in range(2)]
    for x, y in zip(*runs):
        assert x.tobytes() == y.tobytes()
    coords, numsteps, ray_indices, counters = runs[0]
    want_numsteps, want_idx, want_counters, _ = ref.layout_from_counts(counts, max_samples)
    emitted = int(counters[0])
    assert tuple(int(v) for v in counters) == want_counters and (emitted < (counts > 0).sum()) == cut
    if cut:
        assert want_idx[-1] < k and ((counts[want_idx[-1] + 1:k] == 0).all())
    assert (numsteps[:emitted] == want_numsteps).all() and (ray_indices[:emitted] == want_idx).all()
    assert (numsteps[emitted:] == 0).all() and (ray_indices[emitted:] == 0).all()
    want_coords = np.zeros_like(coords)
    end = int(want_numsteps[-1].sum())
    want_coords[:end] = np.concatenate([records[i % 100] for i in want_idx])   # (bases are the running sum: the emitted rays' records lie back to back)
    assert coords.tobytes() == want_coords.tobytes(), "records of ray i are those of ray i % 100; zero behind the last emitted ray"


# ---- torch -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_ray_loss_function_and_ray_step(ctx, generated, scene):
    """torch_module.ray_loss differentiates the mean loss with respect to the outputs (the kernel's dL/doutput over the loss scale, scattered back to the samples'
    rows), and NerfNetworkModule.ray_step leaves the same parameter gradient as forward -> ray_loss -> backward; a few Adam steps lower the loss."""
    from nerfshop_amd import _abi, synth, torch_module
    net, rays, jitter, walk, counts, stable = generated
    coords, numsteps, ray_indices, counters = net.training_samples(None, torch.from_numpy(rays).to(DEV), torch.from_numpy(jitter).to(DEV), 0.0, 20000)
    emitted, n = int(counters[0]), int(counters[1])
    assert n <= 20000
    numsteps, coords = numsteps[:emitted].contiguous(), coords[:n].contiguous()
    rng = np.random.default_rng(2)
    target = torch.from_numpy(np.concatenate([rng.random((emitted, 3)), np.ones((emitted, 1))], 1).astype(np.float32)).to(DEV)
    module = torch_module.NerfNetworkModule(desc=synth.model_desc(1, log2_hashmap_size=14), seed=5, ctx=ctx)
    params = _abi.RayLossParams(max_samples_compacted=n + 64)
    module.zero_grad()
    outputs = module(coords)
    outputs.retain_grad()
    loss = torch_module.ray_loss(outputs, coords, numsteps, target, module.network, params)
    loss.backward()
    manual = module.params.grad.clone()
    # the derivative with respect to the outputs, against the twin on the very outputs the network gave
    b = dict(out=outputs.detach()[:, :4].double().cpu().numpy(), coords=coords.cpu().numpy(), numsteps=numsteps.cpu().numpy().astype(np.int64), target=target.cpu().numpy(),
             background=None, origins=None, rgb_act=ref.ACT_LOGISTIC, den_act=ref.ACT_EXPONENTIAL, aabb=ref.AABB_UNIT,
             p=dict(loss_type=ref.L2, color_space=ref.LINEAR, lin=False, loss_scale=128.0, background=(0.0, 0.0, 0.0), near_distance=0.0, l1=False, cap=n + 64))
    c = ref.closed_form(b)
    np.testing.assert_allclose(float(loss.detach()), float(c.loss.sum()), rtol=1e-5)
    want = np.zeros((n, 4))
    used = (c.src >= 0).numpy()
    want[c.src.numpy()[used]] = c.dl.numpy()[used] / 128.0
    got = outputs.grad[:, :4].double().cpu().numpy()
    assert float(outputs.grad[:, 4:].abs().max()) == 0
    scale = np.abs(want).max()
    assert scale > 0 and np.abs(got - want).max() <= 2e-3 * scale
    module.zero_grad()
    fused = module.ray_step(coords, numsteps, target, params)
    np.testing.assert_allclose(float(fused), float(loss.detach()), rtol=1e-6)
    g = module.params.grad
    assert float((g - manual).abs().max()) <= 1e-3 * float(manual.abs().max()) and float(manual.abs().max()) > 0
    opt = torch.optim.Adam(module.parameters(), lr=1e-2, eps=1e-15)
    history = []
    for _ in range(12):
        opt.zero_grad()
        history.append(float(module.ray_step(coords, numsteps, target, params)))
        opt.step()
    print("ray_step losses:", " ".join(f"{v:.5f}" for v in history))
    assert history[-1] < history[0]
