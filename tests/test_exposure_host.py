"""Per-image exposure without a GPU: the surface, nrs_exposure_step_host against the twin (tests/exposure_ref.py), and the refusals that need no device.  Every test
that touches the library fails without the feature (the symbols are missing).

Bars for the step, tests/test_gpu_optimizer.py's for the same fp32 operations: values, m and v against the float64 twin in fp32 steps of the exact element, at most
4 x the worst error of the float32 twin on the same inputs plus one step; and, as there, bit-equal to the float32 twin (IEEE division and square root, no
contraction, the same order).  Every step is judged from the state the library itself left before it.  The values are judged behind the renormalisation's
subtraction, where value - mean cancels: their error is measured in float32 steps of twice the largest value."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import exposure_ref as ref
import optimizer_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
f32 = np.float32
ONE = 1 << 32


def test_surface_exists(built):
    from nerfshop_amd import _abi, runtime, trainer
    lib = _abi.load()
    header = open(os.path.join(ROOT, "include", "nrs.h")).read()
    for name in ("nrs_exposure_default_params", "nrs_exposure_create", "nrs_exposure_destroy", "nrs_exposure_n_images", "nrs_exposure_step_count", "nrs_exposure_set",
                 "nrs_exposure_get", "nrs_exposure_export", "nrs_exposure_targets", "nrs_exposure_accumulate", "nrs_exposure_step", "nrs_exposure_step_host"):
        assert name in _abi.EXPORTS and hasattr(lib, name) and f"{name}(" in header, name
    assert lib.nrs_abi_version() == 3, "new surface, detected by symbol: no existing layout changes"
    assert C.sizeof(_abi.RayLossParams) == 44 and C.sizeof(_abi.AdamParams) == 28 and C.sizeof(_abi.EnvmapAccumulateParams) == 20, "the existing structs keep their bits"
    assert C.sizeof(_abi.ExposureParams) == 24 == _abi.ExposureParams().struct_size
    assert C.sizeof(_abi.ExposureAccumulateParams) == 12 == _abi.ExposureAccumulateParams().struct_size
    p = _abi.ExposureParams(beta1=0.0, beta2=0.0, epsilon=1.0, l2_reg=1.0, steps_between_updates=1)
    lib.nrs_exposure_default_params(C.byref(p))
    assert (p.struct_size, p.beta1, p.beta2, p.epsilon, p.l2_reg, p.steps_between_updates) == (24, f32(0.9), f32(0.99), f32(1e-8), 0.0, 16)
    assert bytes(p) == bytes(_abi.ExposureParams()), "the ctypes default is the library's"
    assert (_abi.EXPOSURE_VALUES, _abi.EXPOSURE_M, _abi.EXPOSURE_V, _abi.EXPOSURE_CELLS, _abi.EXPOSURE_GRADIENT) == (0, 1, 2, 3, 4)
    for word in ("NRS_EXPOSURE_VALUES = 0", "NRS_EXPOSURE_M = 1", "NRS_EXPOSURE_V = 2", "NRS_EXPOSURE_CELLS = 3", "NRS_EXPOSURE_GRADIENT = 4"):
        assert word in header, word
    assert "Not here: exposure" not in header and "Not here: per-image exposure" not in header and "distortion map, exposure (" not in header, \
        "the three 'Not here' sentences lose exposure"
    for method in ("set", "get", "export", "targets", "accumulate", "step", "step_count"):
        assert callable(getattr(runtime.Exposure, method))
    sig = inspect.signature(trainer.Trainer.__init__).parameters
    assert sig["exposure"].default is None and sig["exposure_l2_reg"].default == 0.0 and sig["cam_update_every"].default == 16
    sig = inspect.signature(trainer.Trainer.step).parameters
    assert sig["pixels"].default is None and sig["xy_pdf"].default is None
    assert callable(trainer.Trainer.exposures)
    compat = open(os.path.join(ROOT, "include", "nrs_compat.hpp")).read()
    for name in ("class Exposure", "nrs_exposure_targets", "nrs_exposure_accumulate", "nrs_exposure_step", "nrs_exposure_set"):
        assert name in compat, name
    for doc, word in (("README.md", "er-image exposure"), ("DESIGN.md", "Per-image exposure"), ("INTEGRATION.md", "xposure")):
        assert word in open(os.path.join(ROOT, doc)).read(), doc


# ---- the step's host twin -------------------------------------------------------------------------------------------------------------------------------------------
def random_state(rng, n_images):
    """exposures of a few tenths, first moments of either sign, second moments consistent with them"""
    values = (rng.normal(size=(n_images, 3)) * 0.3).astype(f32)
    m = (rng.normal(size=(n_images, 3)) * 1e-2).astype(f32)
    v = ((m.astype(np.float64) ** 2) * rng.uniform(0.5, 20.0, size=(n_images, 3))).astype(f32)
    return values, m, v


def random_cells(rng, n_images, extreme=False):
    """gradients of mixed size; about a third of the images have no rays at all (all three cells zero); extreme: every cell at +-512 * 2^32 * 100"""
    if extreme:
        return (rng.choice([-1, 1], size=(n_images, 3)) * (512 * ONE * 100)).astype(np.int64)
    cells = np.rint(rng.normal(size=(n_images, 3)) * np.exp(rng.uniform(-12, 3, size=(n_images, 1))) * ONE).astype(np.int64)
    cells[rng.random(n_images) < 0.34] = 0
    return cells


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def judge(before, after, cells, t_before, loss_scale, lr, hyper, worst):
    from nerfshop_amd import _abi
    t32 = ref.step(cells, *before, t_before, loss_scale, lr, **hyper)
    t64 = ref.step(cells, *before, t_before, loss_scale, lr, dtype=np.float64, **hyper)
    assert not after[0].any(), "the cells are zero afterwards"
    assert after[4] == t_before + 1
    for k, name in ((2, "m"), (3, "v")):
        e_lib = float(optimizer_ref.ulp_error(after[k], t64[k]).max())
        e_32 = float(optimizer_ref.ulp_error(t32[k], t64[k]).max())
        worst[name] = (max(worst[name][0], e_lib), max(worst[name][1], e_32))
        assert e_lib <= 4.0 * e_32 + 1.0, (name, e_lib, e_32)
    # the values after the subtraction, in float32 steps of the largest value (value - mean cancels)
    size = np.spacing(f32(np.abs(t64[1]).max() + np.abs(t64[1]).max()))
    e_lib = float((np.abs(after[1].astype(np.float64) - t64[1]) / size).max())
    e_32 = float((np.abs(t32[1].astype(np.float64) - t64[1]) / size).max())
    worst["values"] = (max(worst["values"][0], e_lib), max(worst["values"][1], e_32))
    assert e_lib <= 4.0 * e_32 + 1.0, ("values", e_lib, e_32)
    for k, name in ((1, "values"), (2, "m"), (3, "v")):
        assert (bits(after[k]) == bits(t32[k])).all(), f"{name} is bit-equal to the float32 twin"
    # the renormalisation: per channel the values sum to (almost) nothing
    n_images = cells.shape[0]
    total = np.abs(after[1].astype(np.float64).sum(axis=0))
    assert (total <= n_images * np.spacing(f32(np.abs(after[1]).max()))).all(), "the per-channel sum is within n_images float32 steps of the largest value"


@pytest.mark.parametrize("n_images", [1, 3, 257, 2500])
@pytest.mark.parametrize("l2_reg", [0.0, 0.1])
def test_step_host_against_the_twin(built, n_images, l2_reg):
    """1, 3 and 257 images (and 2500: more images than the 1024 partial sums of the mean), from the steps 0, 1 and 99 (t = 1, 2, 100), three steps in a row from
    each; images without rays (zero cells) still move, by momentum and the renormalisation; cells at +-512 * 2^32 * 100 in the last step."""
    from nerfshop_amd import _abi, runtime
    rng = np.random.default_rng(100 * n_images + int(10 * l2_reg))
    hyper = dict(l2_reg=l2_reg)
    params = _abi.ExposureParams(l2_reg=l2_reg)
    loss_scale, lr = 128.0, 1e-2
    worst = dict(values=(0.0, 0.0), m=(0.0, 0.0), v=(0.0, 0.0))
    for t0 in (0, 1, 99):
        state = random_state(rng, n_images) if t0 else tuple(np.zeros((n_images, 3), f32) for _ in range(3))
        t = t0
        for k in range(3):
            cells = random_cells(rng, n_images, extreme=(k == 2))
            after = runtime.exposure_step_host(cells, *state, t, loss_scale, lr, params=params)
            judge(state, after, cells, t, loss_scale, lr, hyper, worst)
            no_rays = ~cells.any(axis=1)
            if t0 and n_images > 1 and no_rays.any():
                assert (bits(after[1])[no_rays] != bits(state[0])[no_rays]).any(), "an image without rays still steps"
                assert (bits(after[2])[no_rays] != bits(state[1])[no_rays]).all() and (bits(after[3])[no_rays] != bits(state[2])[no_rays]).all(), "its moments decay"
            state, t = after[1:4], after[4]
    print(f"n_images={n_images} l2_reg={l2_reg}: worst error in fp32 steps, library / twin32: " + "  ".join(f"{k} {a:.2f} / {b:.2f}" for k, (a, b) in worst.items()))


def test_one_image_renormalises_to_zero(built):
    from nerfshop_amd import runtime
    after = runtime.exposure_step_host(np.array([[ONE, -3 * ONE, 0]]), *(np.zeros((1, 3), f32) for _ in range(3)), 0, 128.0, 1e-2)
    assert (after[1] == 0).all() and (after[2] != 0)[0, :2].all() and after[2][0, 2] == 0 and after[4] == 1, "one image: the mean is the value itself"


def unit_ratio_moments(beta1, beta2, epsilon):
    """(m, v) float32 with fl(beta1 m) == fl(sqrtf(fl(beta2 v)) + epsilon): a zero gradient then moves the value by exactly -alr"""
    b1, b2, eps = f32(beta1), f32(beta2), f32(epsilon)
    for v in (f32(x) for x in (1.0, 2.0, 3.0, 5.0, 7.0, 0.3, 11.0, 13.0)):
        d = f32(np.sqrt(f32(b2 * v)) + eps)
        m = f32(d / b1)
        for cand in (m, np.nextafter(m, f32(0)), np.nextafter(m, f32(1e9)), np.nextafter(np.nextafter(m, f32(0)), f32(0)), np.nextafter(np.nextafter(m, f32(1e9)), f32(1e9))):
            if f32(b1 * cand) == d:
                return cand, v
    raise AssertionError("no such pair")


@pytest.mark.parametrize("betas", [(0.9, 0.99), (0.5, 0.5), (0.8, 0.9)])
@pytest.mark.parametrize("t", [1, 2, 100, 5000])
def test_alr_within_one_ulp(built, betas, t):
    """alr = lr sqrt(1 - beta2^t) / (1 - beta1^t), evaluated in float64 and rounded once, read off a step: two images, zero cells, no l2; image 0 holds moments whose
    decayed ratio m / (sqrt(v) + epsilon) is exactly 1, image 1 holds none.  Image 0 moves by -alr, the mean is -alr / 2 (exact), and the values end as -+alr / 2."""
    from nerfshop_amd import _abi, runtime
    lr = 3.7e-3
    m0, v0 = unit_ratio_moments(betas[0], betas[1], 1e-8)
    m, v = np.zeros((2, 3), f32), np.zeros((2, 3), f32)
    m[0], v[0] = m0, v0
    params = _abi.ExposureParams(beta1=betas[0], beta2=betas[1])
    after = runtime.exposure_step_host(np.zeros((2, 3), np.int64), np.zeros((2, 3), f32), m, v, t - 1, 128.0, lr, params=params)
    assert after[4] == t and (after[1][0] == -after[1][1]).all()
    got = 2.0 * after[1][1].astype(np.float64)
    want = ref.alr64(lr, betas[0], betas[1], t)
    err = np.abs(got - want) / np.spacing(f32(want))
    print(f"betas {betas} t {t}: alr {got[0]:.9e}, float64 {want:.9e}, {err.max():.3f} float32 steps")
    assert err.max() <= 1.0
    assert (after[1] == ref.step(np.zeros((2, 3), np.int64), np.zeros((2, 3), f32), m, v, t - 1, 128.0, lr, beta1=betas[0], beta2=betas[1])[1]).all()


@pytest.mark.parametrize("n_images", [2, 3, 257, 1025, 4096])
def test_mean_within_one_ulp(built, n_images):
    """The mean that is subtracted, read off a step that moves nothing (learning rate 0): before - after per image, which is the mean exactly wherever the
    subtraction is exact -- asserted for the image picked: a value of 0, so after = -mean.  Within 1 float32 step of the float64 mean of the float32 values (the
    float64 sum's error is far below a float32 rounding: the two differ at a tie only), and bit-equal to the twin's mean in the header's fixed order."""
    from nerfshop_amd import runtime
    rng = np.random.default_rng(n_images)
    values = (rng.normal(size=(n_images, 3)) * 0.5 + 0.1).astype(f32)
    values[n_images // 2] = 0.0
    z = np.zeros((n_images, 3), f32)
    after = runtime.exposure_step_host(np.zeros((n_images, 3), np.int64), values, z, z, 0, 128.0, 0.0)
    mean = -after[1][n_images // 2]
    exact = values.astype(np.float64).sum(axis=0) / n_images
    err = np.abs(mean.astype(np.float64) - exact) / np.spacing(np.abs(exact).astype(f32))
    print(f"n_images={n_images}: the mean is {err.max():.3f} float32 steps from the float64 mean")
    assert err.max() <= 1.0
    assert (bits(mean) == bits(ref.mean_of(values))).all()
    assert (bits(after[1]) == bits((values - mean).astype(f32))).all()


# ---- the refusals that need no device ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_without_a_device(built):
    from nerfshop_amd import _abi
    lib = _abi.load()
    fake = C.cast(C.create_string_buffer(1024), C.c_void_p)   # a handle of zeros: every refusal below comes before anything behind it is used for a HIP call
    buf = C.create_string_buffer(8192 + 16)
    q = C.c_void_p((C.addressof(buf) + 15) & ~15)              # 16-byte aligned
    q2 = C.c_void_p(q.value + 4096)
    odd = C.c_void_p(q.value + 4)
    out = C.c_void_p()
    err = lambda: lib.nrs_last_error().decode()
    assert lib.nrs_exposure_create(None, 4, None, C.byref(out)) == INVALID and "NULL" in err()
    assert lib.nrs_exposure_create(fake, 4, None, None) == INVALID and "NULL" in err()
    assert lib.nrs_exposure_create(fake, 0, None, C.byref(out)) == INVALID and "n_images" in err()
    assert lib.nrs_exposure_create(fake, (1 << 20) + 1, None, C.byref(out)) == INVALID and "2^20" in err()
    bad_fields = (("struct_size", 20, "struct_size"), ("beta1", 1.0, "beta1"), ("beta1", -0.1, "beta1"), ("beta1", float("nan"), "beta1"), ("beta2", 1.0, "beta2"),
                  ("beta2", -1e-3, "beta2"), ("epsilon", 0.0, "epsilon"), ("epsilon", -1e-8, "epsilon"), ("epsilon", float("inf"), "epsilon"),
                  ("epsilon", float("nan"), "epsilon"), ("l2_reg", -0.1, "l2_reg"), ("l2_reg", float("inf"), "l2_reg"), ("l2_reg", float("nan"), "l2_reg"),
                  ("steps_between_updates", 0, "steps_between_updates"))
    for field, value, word in bad_fields:
        bad = _abi.ExposureParams()
        setattr(bad, field, value)
        assert lib.nrs_exposure_create(fake, 4, C.byref(bad), C.byref(out)) == INVALID and word in err(), (field, value)
    assert not out.value
    lib.nrs_exposure_destroy(None)
    assert lib.nrs_exposure_n_images(None) == 0 and lib.nrs_exposure_step_count(None) == 0
    assert lib.nrs_exposure_set(None, q) == INVALID and "NULL" in err()
    assert lib.nrs_exposure_get(fake, 5, q, 0) == INVALID and "which" in err()
    assert lib.nrs_exposure_get(fake, -1, q, 0) == INVALID and "which" in err()
    assert lib.nrs_exposure_get(None, 0, q, 0) == INVALID and lib.nrs_exposure_get(fake, 0, None, 0) == INVALID and "NULL" in err()
    assert lib.nrs_exposure_get(fake, 0, q, 5) == INVALID and "3 * n_images" in err()
    assert lib.nrs_exposure_export(None, q, None) == INVALID and lib.nrs_exposure_export(fake, None, None) == INVALID and "NULL" in err()
    good = (fake, None, 8, q, q, q, q, q2, q)
    for k in (0, 3, 4, 5, 6, 7, 8):
        args = list(good)
        args[k] = None
        assert lib.nrs_exposure_targets(*args) == INVALID and "NULL" in err(), k
    assert lib.nrs_exposure_targets(fake, None, (1 << 21) + 1, q, q, q, q, q2, q) == INVALID and "2^21" in err()
    assert lib.nrs_exposure_targets(fake, None, 8, q, q, q, q, q2, odd) == INVALID and "aligned" in err()
    assert lib.nrs_exposure_targets(fake, None, 8, q, q, q, q, q, q) == INVALID and "aliases" in err()
    assert lib.nrs_exposure_targets(fake, None, 8, q, q, q, q, C.c_void_p(q.value + 8 * 16 - 4), q) == INVALID and "aliases" in err(), "the last float of the input"
    assert lib.nrs_exposure_targets(fake, None, 8, q, q, q, q2, C.c_void_p(q2.value - 8 * 16 + 4), q) == INVALID and "aliases" in err(), "the first float of the input"
    assert lib.nrs_exposure_targets(fake, None, 0, None, None, None, None, None, None) == 0, "n_rays == 0 is NRS_OK"
    ap = _abi.ExposureAccumulateParams()
    good = (fake, None, C.byref(ap), 8, q, q, q, q, q, None)
    for k in (0, 2, 4, 5, 6, 7, 8):
        args = list(good)
        args[k] = None
        assert lib.nrs_exposure_accumulate(*args) == INVALID and "NULL" in err(), k
    for field, value, word in (("struct_size", 16, "struct_size"), ("loss_scale", float("inf"), "loss_scale"), ("loss_scale", 0.0, "loss_scale"),
                               ("loss_scale", -1.0, "loss_scale"), ("loss_scale", float("nan"), "loss_scale")):
        bad = _abi.ExposureAccumulateParams()
        setattr(bad, field, value)
        assert lib.nrs_exposure_accumulate(fake, None, C.byref(bad), 8, q, q, q, q, q, None) == INVALID and word in err(), (field, value)
    assert lib.nrs_exposure_accumulate(fake, None, C.byref(ap), (1 << 21) + 1, q, q, q, q, q, None) == INVALID and "2^21" in err()
    assert lib.nrs_exposure_accumulate(fake, None, C.byref(ap), 8, q, q, q, odd, q, None) == INVALID and "aligned" in err()
    assert lib.nrs_exposure_accumulate(fake, None, C.byref(ap), 8, q, q, q, q, odd, None) == INVALID and "aligned" in err()
    assert lib.nrs_exposure_accumulate(fake, None, C.byref(ap), 0, None, None, None, None, None, None) == 0, "n_rays == 0 is NRS_OK"
    assert lib.nrs_exposure_step(None, None, 128.0, 1e-2) == INVALID and "NULL" in err()
    for ls, lr, word in ((0.0, 1e-2, "loss_scale"), (-1.0, 1e-2, "loss_scale"), (float("nan"), 1e-2, "loss_scale"), (float("inf"), 1e-2, "loss_scale"),
                         (128.0, -1.0, "learning_rate"), (128.0, float("inf"), "learning_rate"), (128.0, float("nan"), "learning_rate")):
        assert lib.nrs_exposure_step(fake, None, ls, lr) == INVALID and word in err(), (ls, lr)
    # the host twin refuses what create and step refuse
    cells, vals, t = (C.c_int64 * 6)(), (C.c_float * 6)(), C.c_uint32(0)
    host = lambda n, p, ls, lr, *arrays: lib.nrs_exposure_step_host(n, p, ls, lr, *arrays)
    assert host(2, None, 128.0, 1e-2, cells, vals, vals, vals, C.byref(t)) == 0 and t.value == 1
    for k in range(5):
        arrays = [cells, vals, vals, vals, C.byref(t)]
        arrays[k] = None
        assert host(2, None, 128.0, 1e-2, *arrays) == INVALID and "NULL" in err(), k
    assert host(0, None, 128.0, 1e-2, cells, vals, vals, vals, C.byref(t)) == INVALID and "n_images" in err()
    assert host((1 << 20) + 1, None, 128.0, 1e-2, cells, vals, vals, vals, C.byref(t)) == INVALID and "2^20" in err()
    for field, value, word in bad_fields:
        bad = _abi.ExposureParams()
        setattr(bad, field, value)
        assert host(2, C.byref(bad), 128.0, 1e-2, cells, vals, vals, vals, C.byref(t)) == INVALID and word in err(), (field, value)
    assert host(2, None, 0.0, 1e-2, cells, vals, vals, vals, C.byref(t)) == INVALID and "loss_scale" in err()
    assert host(2, None, 128.0, float("nan"), cells, vals, vals, vals, C.byref(t)) == INVALID and "learning_rate" in err()
    assert t.value == 1, "a refused call leaves the step count alone"
