"""nrs_tonemap = CudaRenderBuffer::tonemap (src/render_buffer.cu:562-580; tonemap_kernel :471-501, tonemap and its curves :254-332) and nrs_accumulate_spp_tonemap
on an MI355X against a numpy restatement of the same arithmetic in np.float32, step by step in the reference's order.

The library is compiled with -ffp-contract=off and the kernel holds no fmaf, so everything except the powf of the two sRGB curves is bit-reproducible: cases that
take no sRGB curve compare as uint32 words.  The sRGB curves are evaluated here in float64 and rounded (a correctly rounded powf); cases that take one are held to
|got - ref| <= 2e-6 * max(1, |ref|) -- the bar tests/test_gpu_accumulate.py holds the same device powf to on values <= 1.5, applied relatively above 1 -- and their
alpha, which takes no curve, stays bit-exact whenever the clamp is off (and here also when it is on: the clamp is exact).

RGBA8: byte = floor(clamp(ref) * 255 + 0.5) of the reference, one level of slack only where that value lies within 255 * 2e-6 of an integer (the float tolerance
carried through the quantisation; it also covers the fp32 rounding of c * 255 + 0.5 on the device, <= 2^-16).  Fewer than 1 % of the reference's bytes lie in that band.

The fused call is compared with the pair it replaces (nrs_accumulate_spp, nrs_tonemap), bit for bit, never with itself.  The end-to-end case holds
Testbed.render_to_cpu to the oracle's 8 frames, folded by the oracle's accumulate and tonemapped by the restatement, at the Shade bar (6e-3 max, 2e-4 mean: a mean of frames
that each meet it; the background's weight is <= 1)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
H, W = 53, 77          # 4081 pixels: odd, ragged against the 256-thread workgroups (16 of them)
TOL = 2e-6
LEVEL_BAND = 255 * 2e-6
CURVES = {0: "identity", 1: "aces", 2: "hable", 3: "reinhard"}
BACKGROUNDS = ((0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0, 1.0), (0.2, 0.5, 0.8, 0.6))
PLANTED = [F(0.0), F(0.0031308), F(0.04045), F(1.0)]


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------------------------
def srgb_to_linear(s):
    """common_device.cuh:31-37: s <= 0.04045f ? s / 12.92f : powf((s + 0.055f) / 1.055f, 2.4f) -- the fp32 operations in fp32, the pow in float64 and rounded"""
    s = np.asarray(s, F)
    base = (s + F(0.055)) / F(1.055)
    with np.errstate(invalid="ignore"):
        p = np.power(base.astype(np.float64), np.float64(F(2.4))).astype(F)
    return np.where(s <= F(0.04045), s / F(12.92), p).astype(F)


def linear_to_srgb(l):
    """common_device.cuh:55-61: l < 0.0031308f ? 12.92f * l : 1.055f * powf(l, 0.41666f) - 0.055f"""
    l = np.asarray(l, F)
    with np.errstate(invalid="ignore"):
        p = np.power(l.astype(np.float64), np.float64(F(0.41666))).astype(F)
    return np.where(l < F(0.0031308), F(12.92) * l, F(1.055) * p - F(0.055)).astype(F)


def max0(x):   # Array3f::cwiseMax(0.f): (x < 0) ? 0 : x
    return np.where(x < F(0), F(0), x).astype(F)


def min1(x):   # cwiseMin(1.f): (1 < x) ? 1 : x
    return np.where(F(1) < x, F(1), x).astype(F)


def curve_coefficients(curve):
    """k0..k5 of the rational curves in fp32, in the order render_buffer.cu:261-296 derives them"""
    if curve == 1:
        return F(0.6) * F(0.6) * F(2.51), F(0.6) * F(0.03), F(0.0), F(0.6) * F(0.6) * F(2.43), F(0.6) * F(0.59), F(0.14)
    A, B, Cc, D, E, Fc, Wp = F(0.15), F(0.50), F(0.10), F(0.20), F(0.02), F(0.30), F(11.2)
    k0, k1, k2, k3, k4, k5 = A * Fc - A * E, Cc * B * Fc - B * E, F(0.0), A * Fc, B * Fc, D * Fc * Fc
    nom = k0 * (Wp * Wp) + k1 * Wp + k2
    denom = k3 * (Wp * Wp) + k4 * Wp + k5
    white_scale = denom / nom
    return F(4.0) * k0 * white_scale, F(2.0) * k1 * white_scale, k2 * white_scale, F(4.0) * k3, F(2.0) * k4, k5


def tonemap_ref(acc, exposure=0.0, bg=(0, 0, 0, 0), color_space=0, out_space=0, curve=0, clamp=0):
    """tonemap_kernel's per-pixel work (render_buffer.cu:483-495) on acc [..., 4] float32 -> float32"""
    c = np.array(acc, F, copy=True)
    bg = np.asarray(bg, F)
    bg_rgb = bg[:3] if color_space == 1 else srgb_to_linear(bg[:3])
    weight = (F(1) - c[..., 3]) * bg[3]
    rgb = c[..., :3] + bg_rgb * weight[..., None]
    a = c[..., 3] + weight
    if color_space == 1:
        rgb = srgb_to_linear(rgb)
    scale = F(2.0 ** exposure)   # integer exposures: exact
    rgb = (rgb * scale).astype(F)
    if curve != 0:
        rgb = max0(rgb)
        if curve == 3:
            Y = (F(0.2126) * rgb[..., 0] + F(0.7152) * rgb[..., 1]) + F(0.0722) * rgb[..., 2]
            rgb = rgb * (F(1) / (Y + F(1)))[..., None]
        else:
            k0, k1, k2, k3, k4, k5 = curve_coefficients(curve)
            sq = rgb * rgb
            rgb = ((sq * k0 + k1 * rgb) + k2) / ((k3 * sq + k4 * rgb) + k5)
    if out_space == 1:
        rgb = linear_to_srgb(rgb)
    out = np.concatenate([rgb.astype(F), a[..., None].astype(F)], axis=-1)
    assert out.dtype == F
    return min1(max0(out)) if clamp else out


def quantise(ref):
    """-> (bytes of the reference, True where one level of slack applies)"""
    v = np.clip(ref.astype(np.float64), 0.0, 1.0) * 255.0 + 0.5
    return np.floor(v).astype(np.uint8), np.abs(v - np.round(v)) <= LEVEL_BAND


def make_input(seed=0, h=H, w=W):
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, 1.5, (h, w, 4)).astype(F)
    a[..., 3] = rng.uniform(0.0, 1.0, (h, w)).astype(F)
    a[::3, ::5, :3] *= F(1e-3)                                     # under the 0.0031308 knee
    if h > 13:
        a[7, :, :3] = -rng.uniform(0.0, 0.5, (w, 3)).astype(F) - F(1e-6)   # one negative row, [-0.5, 0)
        planted = [v for x in PLANTED for v in (np.nextafter(x, F(-np.inf)), x, np.nextafter(x, F(np.inf)))]
        for col, v in enumerate(planted):
            a[11, 1 + col, :3] = v; a[11, 1 + col, 3] = 1.0       # alpha 1: no background reaches them
            a[13, 1 + col, :3] = v; a[13, 1 + col, 3] = 0.0       # alpha 0: all of it does
        a[17, 3, 3] = 0.0; a[17, 4, 3] = 1.0
    return a


# ---- the device ----------------------------------------------------------------------------------------------------------------------------------------------
class Dev:
    def __init__(self, rig):
        from nerfshop_amd import _abi
        self.rig, self.torch, self.abi, self.lib = rig, rig.torch, _abi, _abi.load()

    def params(self, exposure=0.0, bg=(0, 0, 0, 0), color_space=0, out_space=0, curve=0, clamp=0, fmt=0):
        t = self.abi.TonemapParams()
        t.exposure = exposure
        t.background_color[:] = bg
        t.color_space, t.output_color_space, t.tonemap_curve, t.clamp_output, t.output_format = color_space, out_space, curve, clamp, fmt
        return t

    def out_buffer(self, n, fmt, fill):
        """n pixels of output and one guard dword behind them, every dword = fill"""
        words = n * (4 if fmt == 0 else 1) + 1
        return self.torch.full((words,), fill, dtype=self.torch.int32, device="cuda:0")

    def result(self, out, shape, fmt):
        host = out.cpu().numpy()
        guard = host[-1]
        if fmt == 0:
            return host[:-1].view(F).reshape(shape + (4,)), guard
        return host[:-1].view(np.uint8).reshape(shape + (4,)), guard

    def tonemap(self, acc_t, fmt=0, fill=0x5A5A5A5A, **kw):
        h, w = acc_t.shape[:2]
        out = self.out_buffer(h * w, fmt, fill)
        self.abi.check(self.lib.nrs_tonemap(self.rig.ctx.h, None, w, h, acc_t.data_ptr(), C.byref(self.params(fmt=fmt, **kw)), out.data_ptr()))
        self.torch.cuda.synchronize()
        got, guard = self.result(out, (h, w), fmt)
        assert guard == fill, "the dword behind the last pixel was written"
        return got


@pytest.fixture(scope="module")
def dev(rig):
    return Dev(rig)


@pytest.fixture(scope="module")
def planes(dev):
    host = make_input()
    host.setflags(write=False)
    return host, dev.torch.from_numpy(host.copy()).to("cuda:0")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_close(got, ref, what):
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
        bar = TOL * np.maximum(1.0, np.abs(ref.astype(np.float64)))
    assert np.isfinite(ref).all(), what
    assert (err <= bar).all(), (what, float((err / bar).max()), float(err.max()))


# ---- tests ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_restatement_puts_few_bytes_in_the_slack_band():
    """a CPU property of the seeded input, asserted where the RGBA8 cases rely on it"""
    acc = make_input()
    for kw in RGBA8_CASES:
        _, band = quantise(tonemap_ref(acc, **kw))
        assert band.mean() < 0.01, (kw, band.mean())


@pytest.mark.parametrize("curve", list(CURVES), ids=list(CURVES.values()))
def test_linear_cases_are_bit_exact(dev, planes, curve):
    host, acc = planes
    n = 0
    for color_space in (0, 2):
        for exposure in (0.0, -2.0, 3.0):
            for bg in BACKGROUNDS:
                for clamp in (0, 1):
                    kw = dict(exposure=exposure, bg=bg, color_space=color_space, out_space=0, curve=curve, clamp=clamp)
                    got, ref = dev.tonemap(acc, **kw), tonemap_ref(host, **kw)
                    assert np.array_equal(bits(got[..., 3]), bits(ref[..., 3])), (kw, "alpha")
                    if all(v in (0.0, 1.0) for v in bg[:3]):
                        a, b = bits(got), bits(ref)
                        assert np.array_equal(a, b), (kw, int((a != b).sum()), float(np.abs(got - ref).max()))
                    else:   # the background's rgb went through srgb_to_linear's powf
                        assert_close(got[..., :3], ref[..., :3], kw)
                    n += 1
    assert n == 36


def test_identity_passes_the_bits_through(dev, planes):
    host, acc = planes
    got = dev.tonemap(acc, exposure=0.0, bg=(0.3, 0.6, 0.9, 0.0), color_space=0, out_space=0, curve=0, clamp=0)
    assert np.array_equal(bits(got), bits(host))
    assert (host[7, :, :3] < 0).all() and np.array_equal(bits(got[7]), bits(host[7]))   # negatives included


@pytest.mark.parametrize("curve", list(CURVES), ids=list(CURVES.values()))
def test_srgb_cases(dev, planes, curve):
    host, acc = planes
    for color_space, out_space in ((1, 0), (1, 1), (0, 1), (2, 1)):
        for exposure in (0.0, -2.0, 3.0):
            for bg in BACKGROUNDS:
                for clamp in (0, 1):
                    kw = dict(exposure=exposure, bg=bg, color_space=color_space, out_space=out_space, curve=curve, clamp=clamp)
                    got, ref = dev.tonemap(acc, **kw), tonemap_ref(host, **kw)
                    assert_close(got, ref, kw)
                    assert np.array_equal(bits(got[..., 3]), bits(ref[..., 3])), (kw, "alpha")


# Identity linear -> linear (bit-exact floats under the bytes), the dearest configuration, and one of each remaining curve / space
RGBA8_CASES = [
    dict(curve=0, color_space=0, out_space=0, exposure=0.0, bg=(0, 0, 0, 0)),
    dict(curve=2, color_space=1, out_space=1, exposure=0.0, bg=(0.2, 0.5, 0.8, 0.6)),
    dict(curve=1, color_space=0, out_space=1, exposure=-2.0, bg=(1, 1, 1, 1)),
    dict(curve=3, color_space=2, out_space=1, exposure=3.0, bg=(0.2, 0.5, 0.8, 0.6)),
    dict(curve=0, color_space=0, out_space=1, exposure=0.0, bg=(0, 0, 0, 0), clamp=1),
]


@pytest.mark.parametrize("case", range(len(RGBA8_CASES)))
def test_rgba8(dev, planes, case):
    host, acc = planes
    kw = RGBA8_CASES[case]
    got = dev.tonemap(acc, fmt=1, **kw)
    assert got.dtype == np.uint8 and got.shape == (H, W, 4)
    want, band = quantise(tonemap_ref(host, **kw))
    assert band.mean() < 0.01
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert d.max() <= 1, (kw, int(d.max()))
    assert not (d[~band] != 0).any(), (kw, int((d[~band] != 0).sum()))
    # the byte order in memory is R, G, B, A: the planted pixels with alpha 1 / 0 (rows 11 and 13) put 255 / 0 (or the background's alpha) in byte 3 ...
    bg_a = F(kw["bg"][3])
    assert (got[11, 1:13, 3] == 255).all() and (got[13, 1:13, 3] == int(np.floor(np.float64(bg_a) * 255 + 0.5))).all()
    if case == 0:   # ... and, with nothing but the quantisation, a pixel of known colour lands channel by channel
        probe = np.zeros((1, 1, 4), F)
        probe[0, 0] = (0.25, 0.5, 0.75, 1.0)
        px = dev.tonemap(dev.torch.from_numpy(probe).to("cuda:0"), fmt=1, **kw)
        assert px.tobytes() == bytes([64, 128, 191, 255])


def test_one_pixel(dev):
    """1 x 1: a single lane of a single workgroup, both formats"""
    probe = np.zeros((1, 1, 4), F)
    probe[0, 0] = (0.9, 0.004, 1.4, 0.25)
    t = dev.torch.from_numpy(probe).to("cuda:0")
    kw = dict(curve=2, color_space=1, out_space=1, exposure=0.0, bg=(0.2, 0.5, 0.8, 0.6))
    ref = tonemap_ref(probe, **kw)
    assert_close(dev.tonemap(t, **kw), ref, "1x1")
    want, band = quantise(ref)
    d = np.abs(dev.tonemap(t, fmt=1, **kw).astype(np.int32) - want)
    assert d.max() <= 1 and not d[~band].any()


def test_in_place(dev, planes):
    host, acc = planes
    for kw in (dict(curve=2, color_space=1, out_space=1, exposure=0.0, bg=(0.2, 0.5, 0.8, 0.6)), dict(curve=1, color_space=0, out_space=0, exposure=3.0, bg=(1, 1, 1, 1), clamp=1)):
        apart = dev.tonemap(acc, **kw)
        buf = acc.clone()
        dev.abi.check(dev.lib.nrs_tonemap(dev.rig.ctx.h, None, W, H, buf.data_ptr(), C.byref(dev.params(**kw)), buf.data_ptr()))
        dev.torch.cuda.synchronize()
        assert np.array_equal(bits(buf.cpu().numpy()), bits(apart))
        assert not np.array_equal(bits(apart), bits(host))
    with pytest.raises(dev.abi.NrsError, match="d_out"):   # 8-bit output is a quarter of the size: in place is refused
        dev.abi.check(dev.lib.nrs_tonemap(dev.rig.ctx.h, None, W, H, acc.data_ptr(), C.byref(dev.params(fmt=1)), acc.data_ptr()))


@pytest.mark.parametrize("fmt", [0, 1], ids=["rgba32f", "rgba8"])
def test_garbage_output_is_overwritten(dev, planes, fmt):
    """whatever the output held, every pixel is written (two different fills, one result) and nothing behind the last pixel is (the guard dword, checked in Dev.tonemap)"""
    _, acc = planes
    kw = dict(curve=3, color_space=0, out_space=1, exposure=0.0, bg=(0.2, 0.5, 0.8, 0.6))
    a = dev.tonemap(acc, fmt=fmt, fill=0x5A5A5A5A, **kw)
    b = dev.tonemap(acc, fmt=fmt, fill=-1, **kw)   # 0xffffffff: NaN words / 255 bytes
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    if fmt == 0:
        assert np.isfinite(b).all()


@pytest.mark.parametrize("fmt", [0, 1], ids=["rgba32f", "rgba8"])
@pytest.mark.parametrize("color_space", [0, 1, 2])
def test_fused_equals_the_pair(dev, color_space, fmt):
    torch, lib, abi, ctx = dev.torch, dev.lib, dev.abi, dev.rig.ctx
    n = W * H
    stride = n + 37   # slabs further apart than they are long
    g = torch.Generator().manual_seed(23 + color_space)
    for K in (1, 2, 5):
        for sample_count in (0, 3):
            slabs = torch.rand((K, stride, 4), generator=g, dtype=torch.float32) * 1.5
            slabs[:, ::7] *= 1e-3
            slabs[:, ::13] = 0.0
            slabs = slabs.to("cuda:0")
            start = torch.rand((n, 4), generator=g, dtype=torch.float32).to("cuda:0")
            t = dev.params(exposure=1.0, bg=(0.2, 0.5, 0.8, 0.6), color_space=color_space, out_space=(K + sample_count) % 2, curve=(K + color_space) % 4, clamp=K % 2, fmt=fmt)
            pair_acc, fused_acc = start.clone(), start.clone()
            pair_out, fused_out = dev.out_buffer(n, fmt, 0x11111111), dev.out_buffer(n, fmt, 0x22222222)
            abi.check(lib.nrs_accumulate_spp(ctx.h, None, W, H, slabs.data_ptr(), stride, K, pair_acc.data_ptr(), sample_count, color_space))
            abi.check(lib.nrs_tonemap(ctx.h, None, W, H, pair_acc.data_ptr(), C.byref(t), pair_out.data_ptr()))
            abi.check(lib.nrs_accumulate_spp_tonemap(ctx.h, None, W, H, slabs.data_ptr(), stride, K, fused_acc.data_ptr(), sample_count, C.byref(t), fused_out.data_ptr()))
            torch.cuda.synchronize()
            what = f"K {K}, sample_count {sample_count}, color space {color_space}"
            a, b = bits(fused_acc.cpu().numpy()), bits(pair_acc.cpu().numpy())
            assert np.array_equal(a, b), f"{what}: {int((a != b).sum())} words of the accumulate buffer differ from nrs_accumulate_spp"
            assert not np.array_equal(b, bits(start.cpu().numpy()))
            a, b = fused_out.cpu().numpy(), pair_out.cpu().numpy()
            assert a[-1] == 0x22222222 and b[-1] == 0x11111111   # the guard dwords
            assert np.array_equal(a[:-1], b[:-1]), f"{what}: {int((a[:-1] != b[:-1]).sum())} words of the output differ from nrs_tonemap"


def test_render_buffer_mirror(dev, planes):
    """RenderBuffer.tonemap / accumulate_spp_tonemap / the setters are the C calls with the buffer's own state"""
    host, acc = planes
    rt, torch = dev.rig.rt, dev.torch
    buf = rt.RenderBuffer(W, H)
    with pytest.raises(dev.abi.NrsError):
        buf.tonemap(dev.rig.ctx)   # nothing accumulated yet
    buf._accumulate = acc.clone()
    buf.set_spp(4)
    buf.set_tonemap_curve(1)
    assert buf.spp() == 0   # a change resets the accumulation, as CudaRenderBuffer's setters do (render_buffer.h:226-238)
    buf.set_tonemap_curve(1); buf.set_spp(4)
    kw = dict(exposure=-2.0, bg=(1.0, 1.0, 1.0, 1.0), color_space=0, out_space=0, curve=1)
    out = buf.tonemap(dev.rig.ctx, exposure=-2.0, background=(1, 1, 1, 1), output_color_space=0)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and tuple(out.shape) == (H, W, 4) and buf.spp() == 4
    assert np.array_equal(bits(out.cpu().numpy()), bits(tonemap_ref(host, **kw)))
    out8 = buf.tonemap(dev.rig.ctx, exposure=-2.0, background=(1, 1, 1, 1), output_color_space=0, fmt="rgba8")
    assert out8.dtype == torch.uint8 and tuple(out8.shape) == (H, W, 4)
    assert np.array_equal(out8.cpu().numpy(), dev.tonemap(acc, fmt=1, **kw))
    with pytest.raises(ValueError):
        buf.tonemap(dev.rig.ctx, fmt="rgb565")
    frames = torch.rand((3, H, W, 4), generator=torch.Generator().manual_seed(3), dtype=torch.float32).to("cuda:0")
    other = rt.RenderBuffer(W, H)
    other.set_tonemap_curve(1); other._accumulate = acc.clone(); other.set_spp(4)
    fused = buf.accumulate_spp_tonemap(dev.rig.ctx, frames, exposure=-2.0, background=(1, 1, 1, 1), output_color_space=0)
    other.accumulate_spp(dev.rig.ctx, frames)
    pair = other.tonemap(dev.rig.ctx, exposure=-2.0, background=(1, 1, 1, 1), output_color_space=0)
    torch.cuda.synchronize()
    assert buf.spp() == other.spp() == 7
    assert np.array_equal(bits(fused.cpu().numpy()), bits(pair.cpu().numpy()))
    assert np.array_equal(bits(buf.accumulate_buffer().cpu().numpy()), bits(other.accumulate_buffer().cpu().numpy()))


def test_render_to_cpu_end_to_end(rig):
    """Testbed.render_to_cpu, 160 x 90 at 8 spp on the scene with its cage edit, against the oracle's 8 frames folded by the oracle and tonemapped by the restatement"""
    from oracle import oracle as orc
    rig.use_edit(True)
    tb = rig.testbed
    try:
        tb.snap_to_pixel_centers = False   # the Sobol pixel offsets of spp_index 0..7, as tests/test_gpu_accumulate.py's 8-spp frame
        Wd, Hd, spp = 160, 90, 8
        p = rig.scene.params_for(Wd, Hd, 60.0, snap=False)
        cam = (tuple(p.focal_length), list(p.camera_matrix0), list(p.camera_matrix1), tuple(p.rolling_shutter), tuple(p.screen_center))
        bg = (1.0, 1.0, 1.0, 1.0)
        got = tb.render_to_cpu(rig.net, Wd, Hd, spp, True, *cam, exposure=0.0, background=bg, fmt="rgba32f", tonemap_curve=0)
        assert isinstance(got, np.ndarray) and got.dtype == F and got.shape == (Hd, Wd, 4)
        buf = tb.render_to_cpu_buffer()
        assert buf.spp() == spp
        ref_acc = np.zeros((Hd, Wd, 4), F)
        for k in range(spp):
            buf_k = rig.rt.RenderBuffer(Wd, Hd)
            buf_k.set_spp(k)
            q = tb.make_params(buf_k, *cam, True)   # the very view render_to_cpu rendered, sample k
            assert q.spp_index == k and q.snap_to_pixel_centers == 0
            orc.accumulate(rig.scene.oracle_model.render(q, [rig.scene.oracle_edit])[0], ref_acc, k, 0)
        ref = tonemap_ref(ref_acc, exposure=0.0, bg=bg, color_space=0, out_space=0, curve=0)
        d = np.abs(got - ref)
        print(f"[render_to_cpu] max |d| {d.max():.3e}, mean {d.mean():.3e}")
        assert d.max() < 6e-3 and d.mean() < 2e-4, (d.max(), d.mean())
        assert np.abs(ref_acc[..., 3] - 1).max() > 0.5 and np.abs(got[..., 3] - 1).max() < 1e-5   # the white, opaque background filled what the scene left open
        # on the device's own accumulate buffer the display step is the restatement's, bit for bit
        assert np.array_equal(bits(got), bits(tonemap_ref(buf.accumulate_buffer().cpu().numpy(), exposure=0.0, bg=bg)))

        # 8 bits, sRGB output
        got8 = tb.render_to_cpu(rig.net, Wd, Hd, spp, False, *cam, exposure=0.0, background=(0.0, 0.0, 0.0, 0.0), fmt="rgba8")
        assert isinstance(got8, np.ndarray) and got8.dtype == np.uint8 and got8.shape == (Hd, Wd, 4)
        gotf = tb.render_to_cpu(rig.net, Wd, Hd, spp, False, *cam, exposure=0.0, background=(0.0, 0.0, 0.0, 0.0), fmt="rgba32f")
        alpha_levels = np.clip(gotf[..., 3].astype(np.float64), 0, 1) * 255
        assert np.abs(got8[..., 3].astype(np.float64) - alpha_levels).max() <= 2
        again = tb.render_to_cpu_buffer().tonemap(rig.ctx, exposure=0.0, background=(0, 0, 0, 0), output_color_space=1, fmt="rgba8")
        rig.torch.cuda.synchronize()
        assert np.array_equal(got8, again.cpu().numpy())
    finally:
        tb.snap_to_pixel_centers = True
        rig.use_edit(False)
