"""The dataset without a GPU: the host skip-ahead against the oracle's, the transforms.json loader against the twin reader of tests/dataset_ref.py (cameras bit for bit,
pixels byte for byte), the loader's refusals, the reference's fox poses (tests/golden/fox_transforms.json, a copy of data/nerf/fox/transforms.json: settings and poses
only), the C-ABI refusals that need no device, and the CPU side of two bars the GPU tests use (the conversion's and mark_untrained's).

Every test that touches the library or nerfshop_amd/dataset.py fails without the feature; test_conversion_bar_on_the_cpu and
test_mark_untrained_cameras_stay_under_the_cap pin the twins and the inputs of the GPU tests alone."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import dataset_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOX = os.path.join(ROOT, "tests", "golden", "fox_transforms.json")
INVALID, STATE = -1, -5


def test_surface_exists(built):
    from nerfshop_amd import _abi, dataset, runtime, trainer
    lib = _abi.load()
    header = open(os.path.join(ROOT, "include", "nrs.h")).read()
    for name in ("nrs_dataset_create", "nrs_dataset_destroy", "nrs_dataset_set_image", "nrs_dataset_set_camera", "nrs_dataset_get_image", "nrs_dataset_rays", "nrs_dataset_mark_untrained",
                 "nrs_rng_advance"):
        assert name in _abi.EXPORTS and hasattr(lib, name) and f"{name}(" in header, name
    assert lib.nrs_abi_version() == 3 and "#define NRS_ABI_VERSION 3 " in header
    assert C.sizeof(_abi.TrainingCamera) == 164 == _abi.TrainingCamera().struct_size
    assert C.sizeof(_abi.DatasetRaysParams) == 32 == _abi.DatasetRaysParams().struct_size
    assert _abi.RNG_STEP_DELTA == 1 << 32 and "#define NRS_RNG_STEP_DELTA (1ull << 32)" in header
    for method in ("set_image", "set_camera", "rays", "mark_untrained"):
        assert callable(getattr(runtime.Dataset, method))
    assert callable(trainer.Trainer.step_dataset) and callable(trainer.Trainer.fit) and callable(dataset.load_transforms)
    assert "testbed.h:584" in runtime.Dataset.rays.__doc__ and "testbed.h:584" in trainer.Trainer.step_dataset.__doc__


@pytest.mark.parametrize("delta", [0, 1, 8, 1 << 32, (1 << 63) + 5])
def test_rng_advance_against_the_oracle(built, delta):
    from nerfshop_amd import _abi, runtime
    from oracle import oracle as orc
    lib = _abi.load()
    for seed in (1337, 11):
        st, inc = C.c_uint64(), C.c_uint64()
        lib.nrs_rng_seed(seed, C.byref(st), C.byref(inc))
        o = orc.Pcg32(seed)
        assert (st.value, inc.value) == (o.state.value, o.inc.value)
        o.next_uint()  # not at the seed's own state
        st.value = o.state.value
        o.advance(delta)
        lib.nrs_rng_advance(C.byref(st), inc.value, delta)
        assert st.value == o.state.value
        assert runtime.rng_advance(st.value, inc.value, 0) == st.value
    lib.nrs_rng_advance(None, 3, 1)  # a NULL state is left alone


# ---- the loader ------------------------------------------------------------------------------------------------------------------------------------------------
def _pose(k):
    a = 0.4 * k + 0.1
    r = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]) @ np.array([[1.0, 0.0, 0.0], [0.0, 0.6, -0.8], [0.0, 0.8, 0.6]])
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = r, (1.5 * np.cos(a), 1.5 * np.sin(a), 0.7 + 0.1 * k)
    return m.tolist()


def write_folder(tmp_path, sizes=((5, 3),) * 3, extra=None, drop=None):
    from PIL import Image
    rng = np.random.default_rng(5)
    frames, pixels = [], []
    for k, (w, h) in enumerate(sizes):
        a = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        pixels.append(a)
        Image.fromarray(a, "RGBA").save(tmp_path / f"r_{k}.png")
        frames.append({"file_path": f"r_{k}" if k else f"r_{k}.png", "transform_matrix": _pose(k)})   # one path with, the others without the extension
    frames[1] = {"file_path": "r_1", "transform_matrix_start": _pose(1), "transform_matrix_end": _pose(4)}
    js = {"camera_angle_x": 0.9, "fl_y": 7.25, "cx": 2.75, "cy": 1.25, "w": 5, "h": 3, "aabb_scale": 2, "scale": 0.4, "offset": [0.5, 0.45, 0.55], "k2": 0.01,
          "rolling_shutter": [0.1, 0.2, 0.3], "white_transparent": True, "frames": frames}
    js.update(extra or {})
    for key in drop or ():
        del js[key]
    (tmp_path / "transforms.json").write_text(json.dumps(js))
    return pixels


def test_loader_against_the_twin_reader(built, tmp_path):
    from nerfshop_amd import dataset
    pixels = write_folder(tmp_path)
    got = dataset.load_transforms(str(tmp_path))
    want = ref.read_transforms(str(tmp_path))
    assert got.n_images == 3 and (got.width, got.height) == (5, 3) == (want["width"], want["height"])
    assert (got.aabb_scale, got.white_transparent, got.black_transparent) == (2, True, False)
    assert got.scale == pytest.approx(0.4) and got.offset == pytest.approx((0.5, 0.45, 0.55))
    assert got.paths == want["paths"]
    for k in range(3):
        rec = ref.from_struct(got.cameras[k])
        assert (rec == want["cameras"][k].view(np.uint32)).all(), k
        assert got.images[k].dtype == np.uint8 and got.images[k].tobytes() == pixels[k].tobytes()
    c0, c1 = want["cameras"][0], want["cameras"][1]
    assert (c0[0:12] == c0[12:24]).all() and (c1[0:12] != c1[12:24]).any()          # the frame with _start / _end moves
    assert c0[26] == np.float32(2.75) / np.float32(5) and c0[27] == np.float32(1.25) / np.float32(3)   # off-centre principal point
    assert c0[25] == np.float32(7.25) and c0[24] != c0[25] and c0[24] == pytest.approx(0.5 * 5 / np.tan(0.45), rel=1e-6)
    assert int(c0[32:33].view(np.uint32)[0]) == 1 and c0[34] == np.float32(0.01) and (c0[28:32] == np.array([0.1, 0.2, 0.3, 0.0], np.float32)).all()
    # the file itself is as good as its folder; n_frames culls; the metadata-only load needs no image
    assert dataset.load_transforms(str(tmp_path / "transforms.json")).n_images == 3
    write_folder(tmp_path, extra={"n_frames": 2, "ftheta_p0": 0.0, "ftheta_p1": 0.001, "ftheta_p2": 0.0, "ftheta_p3": 0.0, "ftheta_p4": 0.0})
    got, want = dataset.load_transforms(str(tmp_path), load_images=False), ref.read_transforms(str(tmp_path))
    assert got.n_images == 2 and got.images is None
    assert got.cameras[0].distortion_mode == 2 and list(got.cameras[0].distortion_params)[4:] == [0.0, 5.0, 3.0]
    assert all((ref.from_struct(got.cameras[k]) == want["cameras"][k].view(np.uint32)).all() for k in range(2))


def test_loader_refusals(built, tmp_path):
    from nerfshop_amd import dataset
    from nerfshop_amd._abi import NrsError
    write_folder(tmp_path, sizes=((5, 3), (5, 3), (4, 3)))
    with pytest.raises(NrsError, match="r_2.png"):
        dataset.load_transforms(str(tmp_path))
    write_folder(tmp_path)
    os.remove(tmp_path / "r_1.png")
    with pytest.raises(NrsError, match="r_1.png"):
        dataset.load_transforms(str(tmp_path))
    (tmp_path / "r_1.png").write_bytes(b"not a png")
    with pytest.raises(NrsError, match="r_1.png"):
        dataset.load_transforms(str(tmp_path))
    write_folder(tmp_path, drop=("frames",))
    with pytest.raises(NrsError, match="frames"):
        dataset.load_transforms(str(tmp_path))
    write_folder(tmp_path, drop=("camera_angle_x", "fl_y"))
    with pytest.raises(NrsError, match="focal"):
        dataset.load_transforms(str(tmp_path))
    with pytest.raises(NrsError, match="cannot read"):
        dataset.load_transforms(str(tmp_path / "nothing_here"))
    write_folder(tmp_path, drop=("w",))
    with pytest.raises(NrsError):   # no images and no resolution
        dataset.load_transforms(str(tmp_path), load_images=False)


def test_fox_poses(built):
    from nerfshop_amd import dataset
    js = json.load(open(FOX))
    got = dataset.load_transforms(FOX, load_images=False)
    want = ref.read_transforms(FOX)
    assert got.n_images == 67 == len(js["frames"]) and got.images is None   # (the file lists 67 frames; the reference's folder ships the images of 50 of them)
    assert (got.width, got.height, got.aabb_scale) == (1080, 1920, 4) == (int(js["w"]), int(js["h"]), js["aabb_scale"])
    f = np.float32
    for k, cam in enumerate(got.cameras):
        assert cam.distortion_mode == 1
        assert [f(v) for v in list(cam.distortion_params)[:4]] == [f(js[n]) for n in ("k1", "k2", "p1", "p2")] and list(cam.distortion_params)[4:] == [0.0, 0.0, 0.0]
        assert f(cam.principal_point[0]) == f(js["cx"]) / f(js["w"]) and f(cam.principal_point[1]) == f(js["cy"]) / f(js["h"])
        assert (f(cam.focal_length[0]), f(cam.focal_length[1])) == (f(js["fl_x"]), f(js["fl_y"]))
        assert list(cam.rolling_shutter) == [0.0] * 4
        assert (ref.from_struct(cam) == want["cameras"][k].view(np.uint32)).all(), k
        assert list(cam.xform_start) == list(cam.xform_end)
    # the pose itself, once by hand: NerfDataset::nerf_matrix_to_ngp on frame 0
    m = np.array(js["frames"][0]["transform_matrix"], np.float32)
    origin = m[:3, 3] * f(0.33) + f(0.5)
    assert list(got.cameras[0].xform_start)[9:12] == [origin[1], origin[2], origin[0]]
    assert list(got.cameras[0].xform_start)[0:3] == [m[1, 0], m[2, 0], m[0, 0]] and list(got.cameras[0].xform_start)[3:6] == [-m[1, 1], -m[2, 1], -m[0, 1]]
    assert got.paths[0].endswith(os.path.join("images", "0001.jpg"))


# ---- C-ABI refusals that need no device --------------------------------------------------------------------------------------------------------------------------
def good_camera():
    return ref.to_struct(ref.camera_record(np.eye(4)[:3], focal=(10.0, 12.0)))


def test_bad_arguments_are_refused_without_a_device(built):
    from nerfshop_amd import _abi
    lib = _abi.load()
    keep = np.zeros(256, np.float32)
    fake = C.c_void_p(keep.ctypes.data)   # a handle of zeros: n_images 0; never used for a device call before the argument checks
    q = keep.ctypes.data
    out = C.c_void_p()

    def refused(status, word, code=INVALID):
        assert status == code and word in lib.nrs_last_error(), (status, lib.nrs_last_error())

    refused(lib.nrs_dataset_create(None, 1, 4, 4, C.byref(out)), b"NULL")
    refused(lib.nrs_dataset_create(fake, 1, 4, 4, None), b"NULL")
    refused(lib.nrs_dataset_create(fake, 0, 4, 4, C.byref(out)), b"n_images")
    refused(lib.nrs_dataset_create(fake, 1, 0, 4, C.byref(out)), b"width or height")
    refused(lib.nrs_dataset_create(fake, 1, 4, 0, C.byref(out)), b"width or height")
    assert not out.value
    lib.nrs_dataset_destroy(None)

    refused(lib.nrs_dataset_set_image(None, 0, 0, q, 0, 0, 0, None), b"NULL")
    refused(lib.nrs_dataset_set_image(fake, 0, 0, None, 0, 0, 0, None), b"NULL")
    refused(lib.nrs_dataset_set_image(fake, 0, 3, q, 0, 0, 0, None), b"format")
    refused(lib.nrs_dataset_set_image(fake, 0, -1, q, 0, 0, 0, None), b"format")
    refused(lib.nrs_dataset_set_image(fake, 0, 0, q, 0, 0, 0, None), b"index")

    refused(lib.nrs_dataset_get_image(None, 0, q), b"NULL")
    refused(lib.nrs_dataset_get_image(fake, 0, None), b"NULL")
    refused(lib.nrs_dataset_get_image(fake, 0, q), b"index")

    cam = good_camera()
    refused(lib.nrs_dataset_set_camera(None, 0, C.byref(cam)), b"NULL")
    refused(lib.nrs_dataset_set_camera(fake, 0, None), b"NULL")
    refused(lib.nrs_dataset_set_camera(fake, 0, C.byref(cam)), b"index")   # a good camera gets as far as the index
    for wrong in (0, 160, 168):
        cam = good_camera()
        cam.struct_size = wrong
        refused(lib.nrs_dataset_set_camera(fake, 0, C.byref(cam)), b"struct_size")
    cam = good_camera()
    cam.distortion_mode = 3
    refused(lib.nrs_dataset_set_camera(fake, 0, C.byref(cam)), b"distortion_mode")
    for field, k, value in (("xform_start", 5, float("nan")), ("xform_end", 11, float("inf")), ("principal_point", 1, float("nan")), ("rolling_shutter", 3, -float("inf")),
                            ("distortion_params", 6, float("nan")), ("focal_length", 0, float("inf"))):
        cam = good_camera()
        getattr(cam, field)[k] = value
        refused(lib.nrs_dataset_set_camera(fake, 0, C.byref(cam)), b"not finite")
    for k, value in ((0, 0.0), (1, -3.0)):
        cam = good_camera()
        cam.focal_length[k] = value
        refused(lib.nrs_dataset_set_camera(fake, 0, C.byref(cam)), b"focal_length")

    p = _abi.DatasetRaysParams()
    rays = lib.nrs_dataset_rays
    refused(rays(None, None, C.byref(p), 1, q, q, q, q, q), b"NULL")
    refused(rays(fake, None, None, 1, q, q, q, q, q), b"NULL")
    for k in (4, 5, 6):
        args = [fake, None, C.byref(p), 1, q, q, q, q, q]
        args[k] = None
        refused(rays(*args), b"NULL")
    p.random_bg_color = 1
    refused(rays(fake, None, C.byref(p), 1, q, q, q, None, q), b"NULL")
    refused(rays(fake, None, C.byref(p), (1 << 21) + 1, q, q, q, q, q), b"2^21")
    p.struct_size = 28
    refused(rays(fake, None, C.byref(p), 1, q, q, q, q, q), b"struct_size")
    # n_rays == 0 is fine, with or without outputs (the handle of zeros has no image left to set)
    p = _abi.DatasetRaysParams()
    assert rays(fake, None, C.byref(p), 0, None, None, None, None, None) == 0
    # a dataset that waits for an image: NRS_ERR_STATE before any device call
    waiting = np.zeros(256, np.uint32)
    waiting[2] = 2   # n_images (behind the context pointer)
    refused(rays(C.c_void_p(waiting.ctypes.data), None, C.byref(p), 1, q, q, q, q, q), b"never been set", STATE)
    refused(lib.nrs_dataset_mark_untrained(None, fake, 1, None), b"NULL")
    refused(lib.nrs_dataset_mark_untrained(fake, None, 1, None), b"NULL")


# ---- the CPU side of two GPU bars ----------------------------------------------------------------------------------------------------------------------------------
def test_conversion_bar_on_the_cpu():
    """Where the GPU test's bar comes from: over every (value, alpha) pair the float32 twin's fp16 result is within one fp16 step of the float64 twin's and differs in
    well under 0.1 % of the elements, also with every power moved by 8 float32 steps (a stand-in for a device powf); alpha is exact."""
    img = ref.all_pairs_image()
    want = ref.from_rgba8_64(img)
    for ulp in (0, 8):
        got = ref.from_rgba8_32(img, perturb_ulp=ulp)
        steps = ref.half_steps(got, want)
        print(f"from_rgba8_32 (+-{ulp} ulp) against from_rgba8_64: {int((steps > 0).sum())} of {steps.size} elements differ ({100.0 * (steps > 0).mean():.4f} %), worst {int(steps.max())} step")
        assert steps.max() <= 1 and (steps > 0).mean() <= 0.001
        assert (got[..., 3].view(np.uint16) == want[..., 3].view(np.uint16)).all()


@pytest.mark.parametrize("aabb_scale", [1, 4])
def test_mark_untrained_cameras_stay_under_the_cap(aabb_scale):
    """The GPU test leaves out cells whose frustum test lies within 1e-6 of its boundary in float64; with these cameras that is far below 0.1 % of the cells, and both
    verdicts occur in bulk."""
    from nerfshop_amd import synth
    grid = ref.marked_grid(aabb_scale)
    kept, _, _ = ref.mark_untrained_ref(grid, ref.corner_cameras(aabb_scale), 48, 32, False)
    bits = np.unpackbits(synth.grid_to_bitfield(kept), bitorder="little")
    assert bits.sum() > 100 and not bits[kept < 0].any(), "the grid of the GPU test: no pooled bit lands in an untrained cell"
    out, near, seen = ref.mark_untrained_ref(grid, ref.corner_cameras(aabb_scale), 48, 32, True)
    for positive, visible in ((True, True), (True, False), (False, True), (False, False)):
        assert (((grid > 0) == positive) & (seen == visible)).sum() > 100, "every branch of the kernel's condition is taken"
    print(f"aabb_scale {aabb_scale}: {int(near.sum())} cells within 1e-6 of the boundary ({100.0 * near.mean():.5f} %), seen {100.0 * seen.mean():.2f} %")
    assert near.mean() <= 0.001
    assert 0.02 < seen.mean() < 0.98
    assert ((out == 0) == seen).all() and ((out == -1) == ~seen).all()
