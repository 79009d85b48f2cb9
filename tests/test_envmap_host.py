"""The trainable environment map without a GPU: the surface, the twin's deposit rule (tests/envmap_ref.py) against hand-worked cells, and the refusals that need no
device.  Every test that touches the library fails without the feature (the symbols are missing); the deposit tests pin the twin the GPU tests compare with."""
import ctypes as C
import inspect
import os

import numpy as np

import envmap_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
f32 = np.float32
ONE = 1 << 32  # a deposit of 1.0


def test_surface_exists(built):
    from nerfshop_amd import _abi, runtime, trainer
    lib = _abi.load()
    header = open(os.path.join(ROOT, "include", "nrs.h")).read()
    for name in ("nrs_envmap_create", "nrs_envmap_destroy", "nrs_envmap_set_texels", "nrs_envmap_get", "nrs_envmap_export", "nrs_envmap_background", "nrs_ray_loss_ex",
                 "nrs_envmap_accumulate", "nrs_envmap_step", "nrs_envmap_resolution", "nrs_envmap_default_adam_params", "nrs_envmap_step_count"):
        assert name in _abi.EXPORTS and hasattr(lib, name) and f"{name}(" in header, name
    assert lib.nrs_abi_version() == 3, "new surface, detected by symbol: no existing layout changes"
    assert C.sizeof(_abi.RayLossParams) == 44 and C.sizeof(_abi.AdamParams) == 28, "nrs_ray_loss and the optimiser keep their structs"
    assert C.sizeof(_abi.EnvmapAccumulateParams) == 20 == _abi.EnvmapAccumulateParams().struct_size
    assert "Not here: the envmap" not in header and "the envmap and exposure" not in header, "the two 'Not here' sentences are updated"
    p = _abi.AdamParams()
    lib.nrs_envmap_default_adam_params(C.byref(p))
    q = _abi.envmap_adam_params()
    assert (p.struct_size, p.beta1, p.beta2, p.epsilon, p.non_matrix_lr_factor, p.ema_decay) == (28, f32(0.9), f32(0.99), f32(1e-10), 1.0, f32(0.99))
    assert bytes(p) == bytes(q), "the ctypes default is the library's"
    assert (_abi.ENVMAP_LEARNING_RATE, _abi.ENVMAP_DECAY_START, _abi.ENVMAP_DECAY_INTERVAL, _abi.ENVMAP_DECAY_BASE) == (1e-2, 10000, 5000, 0.33)
    for method in ("set_texels", "get", "export", "background", "accumulate", "step"):
        assert callable(getattr(runtime.Envmap, method))
    sig = inspect.signature(runtime.NerfNetwork.ray_loss).parameters
    assert sig["background_linear"].default is None and sig["aux"].default is None
    assert inspect.signature(trainer.Trainer.__init__).parameters["envmap"].default is None
    compat = open(os.path.join(ROOT, "include", "nrs_compat.hpp")).read()
    for name in ("class Envmap", "nrs_envmap_background", "nrs_envmap_accumulate", "nrs_envmap_step", "nrs_ray_loss_ex"):
        assert name in compat, name
    for doc, word in (("README.md", "nvironment map"), ("DESIGN.md", "The environment map")):
        assert word in open(os.path.join(ROOT, doc)).read(), doc


# ---- the deposit rule, against hand-worked cells ------------------------------------------------------------------------------------------------------------------
def test_quantise_by_hand():
    q = ref.quantise
    assert q(f32(1.0)) == ONE and q(f32(-0.5)) == -(ONE >> 1) and q(f32(0.25)) == ONE >> 2
    assert q(f32(1000.0)) == 512 * ONE and q(f32(-1e30)) == -512 * ONE, "the clamp, either sign"
    assert q(f32(512.0)) == 512 * ONE and q(np.nextafter(f32(512.0), f32(0))) == 512 * ONE - (1 << 17), "the last float32 below the clamp is exact (2^-15 spacing)"
    assert q(f32("nan")) == 0 and q(f32("inf")) == 0 and q(f32("-inf")) == 0, "non-finite: skipped"
    assert q(f32(0.0)) == 0 and q(f32(-0.0)) == 0
    # ties in the rounding: k + 1/2 units of 2^-32 go to the even neighbour; a float32 holds 2^-33 (1 + 2 j) exactly
    assert q(f32(2.0 ** -33)) == 0, "0.5 -> 0"
    assert q(f32(3 * 2.0 ** -33)) == 2, "1.5 -> 2"
    assert q(f32(5 * 2.0 ** -33)) == 2, "2.5 -> 2"
    assert q(f32(-3 * 2.0 ** -33)) == -2 and q(f32(-5 * 2.0 ** -33)) == -2
    assert q(f32(3 * 2.0 ** -34)) == 1 and q(f32(2.0 ** -34)) == 0, "0.75 -> 1, 0.25 -> 0: a value below half a unit adds nothing"
    assert q(f32(1e-45)) == 0, "a subnormal"


def test_weights_order_and_corners():
    w = ref.weights(f32(0.25), f32(0.5))
    assert [float(x) for x in w] == [0.375, 0.125, 0.375, 0.125]
    assert ref.corners(3, 1, 8, 4) == ((3, 1), (4, 1), (3, 2), (4, 2))
    assert ref.corners(7, 3, 8, 4) == ((7, 3), (0, 3), (7, 3), (0, 3)), "tx + 1 wraps, ty + 1 clamps"
    assert ref.corners(0, 0, 1, 1) == ((0, 0),) * 4, "1 x 1: all four corners are the one texel"
    assert ref.corners(1, 0, 2, 1) == ((1, 0), (0, 0), (1, 0), (0, 0)), "2 x 1: two texels"
    assert ref.corners(-1, -5, 8, 4) == ((7, 0), (0, 0), (7, 0), (0, 0))
    assert ref.corners(1 << 30, 1 << 30, 8, 4) == ((7, 3),) * 4 and ref.corners(-(1 << 31), 0, 8, 4)[0] == (0, 0), "a footprint no lookup wrote stays inside the map"


def test_deposit_by_hand():
    # 8 x 4, one slot at texel (3, 1) with weights (0.25, 0.5), v = (1, -2, 1000): the clamp acts on the product, per deposit
    cells = [0] * (8 * 4 * 4)
    ref.deposit(cells, 8, 4, 3, 1, f32(0.25), f32(0.5), [f32(1.0), f32(-2.0), f32(1000.0)])
    at = lambda x, y, c: cells[4 * (x + y * 8) + c]
    assert [at(3, 1, c) for c in range(4)] == [3 * ONE // 8, -3 * ONE // 4, 375 * ONE, 0]
    assert [at(4, 1, c) for c in range(4)] == [ONE // 8, -ONE // 4, 125 * ONE, 0]
    assert [at(3, 2, c) for c in range(4)] == [3 * ONE // 8, -3 * ONE // 4, 375 * ONE, 0]
    assert [at(4, 2, c) for c in range(4)] == [ONE // 8, -ONE // 4, 125 * ONE, 0]
    assert sum(1 for c in cells if c) == 12
    cells = [0] * (8 * 4 * 4)
    ref.deposit(cells, 8, 4, 3, 1, f32(0.25), f32(0.5), [f32(4000.0), f32("nan"), f32(-0.0)])
    assert [at(3, 1, c) for c in range(4)] == [512 * ONE, 0, 0, 0] and at(4, 1, 0) == 500 * ONE, "1500 clamps to 512, 500 does not; NaN and -0 deposit nothing"
    # 1 x 1: the four products fold onto the one texel, each quantised on its own
    cells = [0] * 4
    ref.deposit(cells, 1, 1, 0, 0, f32(0.25), f32(0.5), [f32(1.0), f32(3 * 2.0 ** -31), f32(0.0)])
    assert cells[0] == ONE
    # 3 * 2^-31 times (0.375, 0.125, 0.375, 0.125) = (2.25, 0.75, 2.25, 0.75) units -> 2 + 1 + 2 + 1, not round(6)
    assert cells[1] == 6 and cells[2] == 0 and cells[3] == 0
    cells = [0] * 4
    ref.deposit(cells, 1, 1, 0, 0, f32(0.5), f32(0.5), [f32(3 * 2.0 ** -31), f32(0.0), f32(0.0)])
    assert cells[0] == 8, "four ties of 1.5 units each round to 2 each: 8, where the exact sum is 6"
    # 2 x 1 at the seam: tx = 1, tx + 1 wraps to 0; the two rows are the same row
    cells = [0] * 8
    ref.deposit(cells, 2, 1, 1, 0, f32(0.25), f32(0.0), [f32(1.0), f32(0.0), f32(0.0)])
    assert cells[4] == 3 * ONE // 4 and cells[0] == ONE // 4 and sum(cells) == ONE, "wy = 0: the second row's weights are 0 and deposit nothing"


def test_cells_to_gradient_and_step_rule():
    g = ref.cells_to_gradient([ONE, -ONE // 2, 3, 0, (1 << 62) + 1])
    assert g.dtype == f32 and [float(x) for x in g[:4]] == [1.0, -0.5, float(f32(3 * 2.0 ** -32)), 0.0] and float(g[4]) == 2.0 ** 30
    # the first step from zero texels: m / sqrt(v) = 0.1 g / (0.1 |g| + epsilon) and bias(1) = 1, so the step is -lr * sign(g) / (1 + 1e-9 / |g|): within 1e-6 of
    # lr for |g| >= 1e-2; untouched where g == 0 (optimizer_ref's rule with the envmap's hyper-parameters)
    st = ref.fresh_state(np.zeros(8, f32))
    grad = np.array([3.0, -0.25, 0.0, -0.0, 1e-2, -1e3, 0.0, 5.0], f32) * f32(128.0)
    out = ref.step(st, grad, 128.0, 1e-2)
    want = -1e-2 * np.sign(grad)
    assert np.abs(out.master - want).max() < 1e-2 * 1e-6 and (out.master[[2, 3, 6]] == 0).all() and (out.steps == (grad != 0)).all()
    assert np.abs(out.ema - out.fp16.astype(np.float64)).max() < 1e-9, "after the first step the EMA is the fp16 copy (a = 0, b = 1)"


# ---- the refusals that need no device ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_without_a_device(built):
    from nerfshop_amd import _abi
    lib = _abi.load()
    fake = C.cast(C.create_string_buffer(1024), C.c_void_p)   # a handle of zeros: every refusal below comes before anything behind it is read or any HIP call
    buf = C.create_string_buffer(4096 + 16)
    q = C.c_void_p((C.addressof(buf) + 15) & ~15)              # 16-byte aligned
    odd = C.c_void_p(q.value + 4)
    out = C.c_void_p()
    err = lambda: lib.nrs_last_error().decode()
    assert lib.nrs_envmap_create(None, 4, 4, None, C.byref(out)) == INVALID and "NULL" in err()
    assert lib.nrs_envmap_create(fake, 4, 4, None, None) == INVALID and "NULL" in err()
    assert lib.nrs_envmap_create(fake, 0, 4, None, C.byref(out)) == INVALID and "resolution" in err()
    assert lib.nrs_envmap_create(fake, 4, 0, None, C.byref(out)) == INVALID and "resolution" in err()
    assert lib.nrs_envmap_create(fake, 1 << 15, (1 << 14) + 1, None, C.byref(out)) == INVALID and "2^31" in err(), "4 * res_x * res_y above 2^31"
    assert lib.nrs_envmap_create(fake, 0xffffffff, 0xffffffff, None, C.byref(out)) == INVALID and "2^31" in err()
    bad = _abi.envmap_adam_params()
    bad.struct_size = 24
    assert lib.nrs_envmap_create(fake, 4, 4, C.byref(bad), C.byref(out)) == INVALID and "struct_size" in err()
    bad = _abi.envmap_adam_params()
    bad.beta2 = 1.0
    assert lib.nrs_envmap_create(fake, 4, 4, C.byref(bad), C.byref(out)) == INVALID and "beta2" in err()
    assert not out.value
    lib.nrs_envmap_destroy(None)
    assert lib.nrs_envmap_set_texels(None, q, 0, None) == INVALID and lib.nrs_envmap_set_texels(fake, None, 0, None) == INVALID and "NULL" in err()
    assert lib.nrs_envmap_get(fake, 4, q, 0) == INVALID and "which" in err()
    assert lib.nrs_envmap_get(fake, -1, q, 0) == INVALID and "which" in err()
    assert lib.nrs_envmap_get(None, 0, q, 0) == INVALID and lib.nrs_envmap_get(fake, 0, None, 0) == INVALID and "NULL" in err()
    assert lib.nrs_envmap_get(fake, 0, q, 5) == INVALID and "4 * res_x * res_y" in err()
    assert lib.nrs_envmap_export(None, 1, q, None) == INVALID and lib.nrs_envmap_export(fake, 1, None, None) == INVALID and "NULL" in err()
    assert lib.nrs_envmap_resolution(None, None, None) == INVALID
    bg3 = (C.c_float * 3)(0.1, 0.2, 0.3)
    good = (fake, None, 8, q, q, q, q, C.byref(bg3), q, q)
    for k in (0, 3, 4, 5, 8, 9):
        args = list(good)
        args[k] = None
        assert lib.nrs_envmap_background(*args) == INVALID and "NULL" in err(), k
    assert lib.nrs_envmap_background(fake, None, 8, q, q, q, None, None, q, q) == INVALID and "default_background" in err()
    assert lib.nrs_envmap_background(fake, None, (1 << 21) + 1, q, q, q, q, C.byref(bg3), q, q) == INVALID and "2^21" in err()
    assert lib.nrs_envmap_background(fake, None, 8, q, q, q, q, C.byref(bg3), q, odd) == INVALID and "aligned" in err()
    assert lib.nrs_envmap_background(fake, None, 0, None, None, None, None, C.byref(bg3), None, None) == 0, "n_rays == 0 is NRS_OK"
    ap = _abi.EnvmapAccumulateParams()
    good = (fake, None, C.byref(ap), 8, q, q, q, q, q)
    for k in (0, 2, 4, 5, 6, 7, 8):
        args = list(good)
        args[k] = None
        assert lib.nrs_envmap_accumulate(*args) == INVALID and "NULL" in err(), k
    for field, value, word in (("struct_size", 16, "struct_size"), ("loss_type", 7, "loss_type"), ("envmap_loss_type", 9, "loss_type"), ("loss_scale", float("inf"), "loss_scale")):
        bad = _abi.EnvmapAccumulateParams()
        setattr(bad, field, value)
        assert lib.nrs_envmap_accumulate(fake, None, C.byref(bad), 8, q, q, q, q, q) == INVALID and word in err(), field
    assert lib.nrs_envmap_accumulate(fake, None, C.byref(ap), (1 << 21) + 1, q, q, q, q, q) == INVALID and "2^21" in err()
    assert lib.nrs_envmap_accumulate(fake, None, C.byref(ap), 8, q, q, odd, q, q) == INVALID and "aligned" in err()
    assert lib.nrs_envmap_accumulate(fake, None, C.byref(ap), 8, q, q, q, q, odd) == INVALID and "aligned" in err()
    assert lib.nrs_envmap_accumulate(fake, None, C.byref(ap), 0, None, None, None, None, None) == 0, "n_rays == 0 is NRS_OK"
    assert lib.nrs_envmap_step(None, None, 128.0, 1e-2) == INVALID and "NULL" in err()
    for ls, lr, word in ((0.0, 1e-2, "loss_scale"), (float("nan"), 1e-2, "loss_scale"), (128.0, -1.0, "learning_rate"), (128.0, float("inf"), "learning_rate")):
        assert lib.nrs_envmap_step(fake, None, ls, lr) == INVALID and word in err(), (ls, lr)
    assert lib.nrs_envmap_step_count(None) == 0
    # nrs_ray_loss_ex refuses what nrs_ray_loss refuses, and a misaligned record
    lp = _abi.RayLossParams(max_samples_compacted=8)
    rl_args = [fake, None, C.byref(lp), 4, None, q, 8, q, 7, q, 16, 1, q, None, None, C.c_void_p(q.value + 64), C.c_void_p(q.value + 2048), q, 16, 1, None, q]
    assert lib.nrs_ray_loss_ex(*rl_args, None, odd) == INVALID and "aligned" in err()
    args = list(rl_args)
    args[2] = None
    assert lib.nrs_ray_loss_ex(*args, None, None) == INVALID and "NULL" in err()
    lp.loss_type = 7
    assert lib.nrs_ray_loss_ex(*rl_args, None, None) == INVALID and "loss_type" in err()
