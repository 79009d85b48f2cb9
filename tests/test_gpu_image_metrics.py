"""nrs_image_metrics / nrs_dataset_image_metrics on an MI355X against the CPU twin (nrs_image_metrics_host) and the float64 restatement of tests/metrics_ref.py, with
the bars of tests/test_metrics_host.py (mean ssim 2e-5 absolute, mse 1e-5 relative, ssim per pixel 1e-3; their origin is written there).  The device and the twin
run the same float32 operations in the same order and differ in powf alone (the device library's against glibc's), so the device is also held to the twin directly,
with the same bars.

Shapes (height, width): 1 x 1, 2 x 3, 5 x 7 (axes shorter than, and about as long as, the blur's reach: every halo pixel is a reflection), 33 x 33 (one pixel more than
the kernel's 32 x 32 tile in each direction: four workgroups, three of them nearly empty), 37 x 53, 67 x 131 (3 x 5 tiles, partial ones on both edges).

The integer sums: two runs give the same bytes; sum_ssim equals the sum of round(ssim_map * 2^32) over the DEVICE'S OWN map exactly, which a lost or a doubled tile
cannot satisfy (every pixel of these images has an ssim far from 0 in sum); sum_sq_err is held to the device's own squared-error map within 2306 n units of 2^-32, the
bound derived in tests/test_metrics_host.py -- the map stores the float32 mean of the three channels, from which the three rounded terms cannot be recovered exactly.
The maps lie between 64 guard floats on either side, which stay as they were."""
import ctypes as C

import numpy as np
import pytest

import metrics_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE = 32
SHAPES = [(1, 1), (2, 3), (5, 7), (TILE + 1, TILE + 1), (37, 53), (67, 131)]
GUARD = 64
GUARD_VALUE = -77.25
f32 = np.float32


@pytest.fixture(scope="module")
def ctx(built):
    from nerfshop_amd import runtime
    return runtime.Context(0)


@pytest.fixture(scope="module")
def cases():
    """per (shape, colour space): the images and, per reference dtype, the twin's answer and the restatement's -- computed once"""
    from nerfshop_amd import runtime
    out = {}
    for shape in SHAPES:
        for color_space in (ref.COLOR_LINEAR, ref.COLOR_SRGB):
            image, reference = ref.make_images(*shape, rgba=color_space == ref.COLOR_SRGB)
            background = (0.0, 0.0, 0.0, 1.0) if color_space == ref.COLOR_LINEAR else (0.2, 0.4, 0.6, 1.0)
            per_dtype = {}
            for dtype in (np.float16, np.float32):
                r = reference.astype(dtype)
                per_dtype[dtype] = (r, runtime.image_metrics_host(image, r, color_space=color_space, background=background, want_maps=True),
                                    ref.metrics(image, r.astype(f32), color_space, background))
            out[shape, color_space] = (image, background, per_dtype)
    return out


def guarded_maps(torch, h, w):
    """two [h, w] float32 views into buffers with GUARD floats of GUARD_VALUE on either side"""
    bufs = [torch.full((h * w + 2 * GUARD,), GUARD_VALUE, dtype=torch.float32, device=DEV) for _ in range(2)]
    return bufs, [b[GUARD:GUARD + h * w].view(h, w) for b in bufs]


def run_device(ctx, image_t, color_space, background, reference_t=None, dataset=None, index=0, maps=True, stream=None):
    """one device call through the C-ABI with guarded maps -> (record as a numpy record, ssim map, sq err map, raw bytes of the record)"""
    import torch
    from nerfshop_amd import _abi
    from nerfshop_amd.runtime import metrics
    from nerfshop_amd.runtime._base import _stream_handle
    h, w = image_t.shape[:2]
    bufs, views = guarded_maps(torch, h, w)
    rec = torch.full((metrics.RECORD_BYTES,), 0xAB, dtype=torch.uint8, device=DEV)   # stale bytes: the call clears its sums itself
    fmt = _abi.IMAGE_RGBA16F_LINEAR if dataset is not None or reference_t.dtype == torch.float16 else _abi.IMAGE_RGBA32F_LINEAR
    p = metrics.metrics_params(color_space, background, fmt)
    m0, m1 = (views[0].data_ptr(), views[1].data_ptr()) if maps else (None, None)
    if dataset is not None:
        _abi.check(ctx.lib.nrs_dataset_image_metrics(dataset.h, index, _stream_handle(stream), image_t.data_ptr(), C.byref(p), rec.data_ptr(), m0, m1))
    else:
        _abi.check(ctx.lib.nrs_image_metrics(ctx.h, _stream_handle(stream), w, h, image_t.data_ptr(), reference_t.data_ptr(), C.byref(p), rec.data_ptr(), m0, m1))
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())
    for b in bufs:
        host = b.cpu().numpy()
        assert (host[:GUARD] == GUARD_VALUE).all() and (host[-GUARD:] == GUARD_VALUE).all(), "a map was written outside its bounds"
        if not maps:
            assert (host == GUARD_VALUE).all()
    raw = rec.cpu().numpy().tobytes()
    return metrics.records_from_bytes(rec)[0], views[0].cpu().numpy(), views[1].cpu().numpy(), raw


@pytest.mark.parametrize("shape", SHAPES)
def test_device_against_twin_and_restatement(ctx, cases, shape):
    import torch
    for color_space in (ref.COLOR_LINEAR, ref.COLOR_SRGB):
        image, background, per_dtype = cases[shape, color_space]
        image_t = torch.from_numpy(image).to(DEV)
        for dtype, (reference, (h_rec, h_ssim, h_sq), want) in per_dtype.items():
            what = f"{shape} colour space {color_space} {np.dtype(dtype).name}"
            rec, ssim_map, sq_map, raw = run_device(ctx, image_t, color_space, background, reference_t=torch.from_numpy(reference).to(DEV))
            ref.check_against_ref(rec, ssim_map, sq_map, want, what + " device / float64")
            twin = dict(n_pixels=int(h_rec["n_pixels"]), ssim=h_rec["ssim"], mse=h_rec["mse"], psnr=h_rec["psnr"], ssim_map=h_ssim.astype(np.float64),
                        sq_err_map=h_sq.astype(np.float64))
            ref.check_against_ref(rec, ssim_map, sq_map, twin, what + " device / twin")
            ref.check_sums_against_maps(rec, ssim_map, sq_map, what)
            # a second run, without maps: the same 32 bytes
            rec2, _, _, raw2 = run_device(ctx, image_t, color_space, background, reference_t=torch.from_numpy(reference).to(DEV), maps=False)
            assert raw2 == raw, what + ": two runs differ"


def test_dataset_images_in_place(ctx, cases):
    """nrs_dataset_image_metrics with image 0 and the last image of a 3-image dataset: the same bytes as nrs_image_metrics on the image read back"""
    import torch
    from nerfshop_amd import runtime
    shape = (67, 131)
    h, w = shape
    ds = runtime.Dataset(ctx, 3, w, h)
    refs = [ref.make_images(h, w, seed=k, rgba=True)[1] for k in range(3)]
    for k in range(3):
        ds.set_image(k, refs[k])   # float32 -> the dataset's fp16
    for color_space in (ref.COLOR_LINEAR, ref.COLOR_SRGB):
        image, background, _ = cases[shape, color_space]
        image_t = torch.from_numpy(image).to(DEV)
        for index in (0, 2):
            stored = ds.get_image(index)
            rec, ssim_map, sq_map, raw = run_device(ctx, image_t, color_space, background, dataset=ds, index=index)
            want = ref.metrics(image, stored.astype(f32), color_space, background)
            ref.check_against_ref(rec, ssim_map, sq_map, want, f"dataset image {index} colour space {color_space}")
            ref.check_sums_against_maps(rec, ssim_map, sq_map, f"dataset image {index}")
            _, _, _, raw_direct = run_device(ctx, image_t, color_space, background, reference_t=torch.from_numpy(stored).to(DEV))
            assert raw == raw_direct
        recs = [run_device(ctx, image_t, color_space, background, dataset=ds, index=k)[3] for k in (0, 1, 2)]
        assert len(set(recs)) == 3, "the three images are three references"
    # the Python face: one evaluation fills one [n, 32] tensor
    out = torch.zeros((3, 32), dtype=torch.uint8, device=DEV)
    image, background, _ = cases[shape, ref.COLOR_LINEAR]
    image_t = torch.from_numpy(image).to(DEV)
    for k in range(3):
        r, m0, m1 = ds.image_metrics(k, image_t, out=out[k], want_maps=(k == 1))
        assert r.data_ptr() == out[k].data_ptr() and (m0 is None) == (k != 1)
    torch.cuda.synchronize()
    recs = runtime.metrics.records_from_bytes(out)
    assert recs.tobytes() == b"".join(run_device(ctx, image_t, ref.COLOR_LINEAR, background, dataset=ds, index=k)[3] for k in range(3))
    s = runtime.metrics_summary(recs)
    want = ref.summary(recs["mse"], recs["ssim"], recs["psnr"])
    assert all(abs(s[k] - want[k]) <= 1e-12 * abs(want[k]) for k in ("psnr_mean", "psnr_min", "psnr_max", "ssim_mean", "psnr_avgmse"))
    ds.close()


def test_identical_images_and_another_stream(ctx, cases):
    import torch
    from nerfshop_amd import runtime
    image, _, _ = cases[(37, 53), ref.COLOR_LINEAR]
    image = np.nan_to_num(image, nan=0.3, posinf=2.0)
    image_t = torch.from_numpy(image).to(DEV)
    rec, ssim_map, _, _ = run_device(ctx, image_t, 0, (0.0, 0.0, 0.0, 1.0), reference_t=image_t.clone())
    assert float(rec["mse"]) == 0.0 and float(rec["psnr"]) == np.inf and float(rec["ssim"]) == 1.0 and (ssim_map == 1.0).all()
    assert int(rec["sum_sq_err"]) == 0 and int(rec["sum_ssim"]) == 37 * 53 << 32
    # a stream other than the default, through both faces
    image, background, per_dtype = cases[(67, 131), ref.COLOR_SRGB]
    reference = per_dtype[np.float16][0]
    image_t, reference_t = torch.from_numpy(image).to(DEV), torch.from_numpy(reference).to(DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    _, _, _, raw_default = run_device(ctx, image_t, ref.COLOR_SRGB, background, reference_t=reference_t)
    _, _, _, raw_side = run_device(ctx, image_t, ref.COLOR_SRGB, background, reference_t=reference_t, stream=side)
    assert raw_side == raw_default
    r, m0, m1 = runtime.image_metrics(ctx, image_t, reference_t, color_space=ref.COLOR_SRGB, background=background, want_maps=True, stream=side)
    side.synchronize()
    assert r.cpu().numpy().tobytes() == raw_default and m0.shape == (67, 131) and m1.shape == (67, 131)


def test_refusals_on_the_device_calls(ctx):
    """every refusal of the two device calls: before any launch, the message names the argument"""
    import torch
    from nerfshop_amd import _abi, runtime
    from nerfshop_amd._abi import NrsError
    lib = ctx.lib
    h, w = 5, 7
    image = torch.zeros((h, w, 4), dtype=torch.float32, device=DEV)
    reference = torch.zeros((h, w, 4), dtype=torch.float32, device=DEV)
    rec = torch.zeros(40, dtype=torch.uint8, device=DEV)

    def call(width=w, height=h, d_image=image.data_ptr(), d_reference=reference.data_ptr(), d_result=rec.data_ptr(), ctx_h=ctx.h, **fields):
        p = _abi.ImageMetricsParams()
        p.reference_format = _abi.IMAGE_RGBA32F_LINEAR
        for k, v in fields.items():
            if k == "background_color":
                p.background_color[:] = v
            else:
                setattr(p, k, v)
        return lib.nrs_image_metrics(ctx_h, None, width, height, d_image, d_reference, C.byref(p), d_result, None, None)
    assert call() == 0
    for kw, word in ((dict(ctx_h=None), b"NULL"), (dict(d_image=None), b"NULL"), (dict(d_reference=None), b"NULL"), (dict(d_result=None), b"NULL"),
                     (dict(width=0), b"is 0"), (dict(height=0), b"is 0"), (dict(width=8193), b"8192"), (dict(height=8193), b"8192"),
                     (dict(struct_size=24), b"struct_size"), (dict(reference_format=_abi.IMAGE_RGBA8_SRGB), b"reference_format"), (dict(reference_format=3), b"reference_format"),
                     (dict(background_color=(float("nan"), 0.0, 0.0, 1.0)), b"finite"), (dict(d_result=rec.data_ptr() + 4), b"misaligned"),
                     (dict(d_image=image.data_ptr() + 4), b"misaligned")):
        assert call(**kw) == -1 and word in lib.nrs_last_error(), (kw, lib.nrs_last_error())
    assert lib.nrs_image_metrics(ctx.h, None, w, h, image.data_ptr(), reference.data_ptr(), None, rec.data_ptr(), None, None) == -1
    ds = runtime.Dataset(ctx, 2, w, h)
    with pytest.raises(NrsError, match="error -1.*index past n_images"):
        ds.image_metrics(2, image)
    with pytest.raises(NrsError, match="error -5.*never been set"):
        ds.image_metrics(1, image)
    ds.set_image(1, np.zeros((h, w, 4), np.float16))
    ds.image_metrics(1, image)
    with pytest.raises(NrsError, match="error -5.*never been set"):
        ds.image_metrics(0, image)
    p = _abi.ImageMetricsParams()
    p.reference_format = _abi.IMAGE_RGBA32F_LINEAR
    assert lib.nrs_dataset_image_metrics(ds.h, 1, None, image.data_ptr(), C.byref(p), rec.data_ptr(), None, None) == -1 and b"reference_format" in lib.nrs_last_error()
    with pytest.raises(NrsError):
        ds.image_metrics(1, torch.zeros((h + 1, w, 4), dtype=torch.float32, device=DEV))   # the wrong shape never reaches the library
    with pytest.raises(NrsError):
        runtime.image_metrics(ctx, image, reference[:, :, :3])
    torch.cuda.synchronize()
    ds.close()
