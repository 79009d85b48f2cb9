"""The optimiser without a GPU: the twins of tests/optimizer_ref.py against each other (the reference's own float32 gap, per array), their skip semantics, the
host-only entry points (nrs_adam_bias_table, nrs_exponential_decay_lr) and every refusal of the new surface that needs no device."""
import ctypes as C
import math

import numpy as np
import pytest

import optimizer_ref as ref


@pytest.fixture(scope="module")
def lib(built):
    from nerfshop_amd import _abi
    return _abi.load()


def last_error(lib):
    return lib.nrs_last_error().decode()


# ---- the twins ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_twin32_against_twin64_on_random_states():
    """The reference's own gap: float32 arithmetic against the real-number rule, per array, in fp32 steps of the exact value.  One step is a handful of correctly
    rounded operations, so a few steps of error -- except where two terms cancel, which costs what the cancellation leaves."""
    hp = ref.Hyper()
    rng = np.random.default_rng(17)
    table = ref.bias_table(hp.beta1, hp.beta2)
    worst = dict(master=0.0, m=0.0, v=0.0, ema=0.0)
    for n, n_matrix in ((4099, 1000), (257, 0), (64, 64)):
        st = ref.random_state(rng, n, n_matrix)
        g = ref.random_grad(rng, n, n_matrix, 128.0)
        a, b = ref.twin64(st, g, hp, n_matrix, 128.0, 1e-2, table), ref.twin32(st, g, hp, n_matrix, 128.0, 1e-2, table)
        assert (a.steps == b.steps).all()
        b_ema = ref.twin64(st, g, hp, n_matrix, 128.0, 1e-2, table, fp16_for_ema=b.fp16).ema
        for k, exact in (("master", a.master), ("m", a.m), ("v", a.v), ("ema", b_ema)):
            worst[k] = max(worst[k], float(ref.ulp_error(getattr(b, k), exact).max()))
        # the stored fp16 of the two twins: equal except at a rounding boundary (at most one fp16 step apart)
        assert float(np.abs(a.fp16.astype(np.float64) - b.fp16.astype(np.float64)).max()) <= float(np.spacing(np.abs(a.fp16)).max())
    print("twin32 vs twin64, worst error in fp32 ulps:", " ".join(f"{k}={v:.2f}" for k, v in worst.items()))
    # v is a sum of non-negative terms, seven roundings deep: no cancellation, so a firm bound (8 = 3.5 relative steps, doubled where the result crosses a binade).
    # m, the weight (its update can be as large as a hash-grid entry) and the EMA are differences of terms of either sign: what float32 costs there is what the
    # cancellation leaves, bounded only by the terms themselves -- recorded, and what the GPU's bar is measured in (tests/test_gpu_optimizer.py).
    assert worst["v"] <= 8.0
    assert all(np.isfinite(x) and x < 2.0 ** 24 for x in worst.values())


@pytest.mark.parametrize("twin", [ref.twin64, ref.twin32])
def test_twin_skip_semantics(twin):
    hp = ref.Hyper(l2_reg=0.5)
    n, n_matrix = 12, 3
    rng = np.random.default_rng(3)
    st = ref.random_state(rng, n, n_matrix)
    st.fp16 = (st.fp16.astype(np.float32) * 3).astype(np.float16)  # not the rounding of master: a skipped element must keep it all the same
    g = np.zeros(n, dtype=np.float32)
    g[5], g[6], g[9] = 1.0, -0.0, 2.0
    out = twin(st, g, hp, n_matrix, 128.0, 1e-2)
    live = np.zeros(n, dtype=bool)
    live[:n_matrix] = True      # matrix weights are never skipped: L2 moves them on a zero gradient
    live[[5, 9]] = True         # -0.0 at 6 counts as zero
    assert (out.steps == st.steps + live).all()
    for k in ("master", "m", "v"):
        assert (getattr(out, k)[~live] == getattr(st, k)[~live]).all() and (getattr(out, k)[live] != getattr(st, k)[live]).all(), k
    assert (out.fp16[~live].view(np.uint16) == st.fp16[~live].view(np.uint16)).all()
    assert (out.fp16[live] == out.master[live].astype(np.float16)).all()
    # the EMA skips nothing
    a, b = ref.ema_coefficients(hp.ema_decay, st.step_count + 1)
    assert (out.ema != st.ema).all() and out.step_count == st.step_count + 1
    np.testing.assert_allclose(out.ema, float(a) * st.ema.astype(np.float64) + float(b) * out.fp16.astype(np.float64), rtol=1e-6)
    # and with ema_decay == 0 it does not move
    assert (twin(st, g, ref.Hyper(ema_decay=0.0), n_matrix, 128.0, 1e-2).ema == st.ema).all()


def test_twin_ema_coefficients_average_the_history():
    """a and b are those of a bias-corrected running mean: T steps on a constant input give that constant, and step 1 forgets the initial value"""
    a, b = ref.ema_coefficients(0.95, 1)
    assert a == 0 and b == 1
    e = 123.0
    for T in range(1, 40):
        a, b = ref.ema_coefficients(0.95, T)
        e = float(a) * e + float(b) * 0.25
        assert abs(e - 0.25) < 1e-6
        assert abs(float(a) + float(b) - 1.0) < 1e-6


# ---- nrs_adam_bias_table -----------------------------------------------------------------------------------------------------------------------------------------
def test_bias_table(lib):
    from nerfshop_amd import runtime
    t = runtime.adam_bias_table(0.9, 0.99)
    want = ref.bias_table(0.9, 0.99)
    print(f"T_sat = {t.size}; bias(1..3) = {t[:3]}")
    assert 1500 < t.size < 1900
    # it ends at the first exact 1.0f of the tail: the last entry is 1, the one before is not
    assert t[-1] == np.float32(1.0) and t[-2] != np.float32(1.0)
    # monotone in the tail: from its minimum on it only rises
    k = int(np.argmin(t))
    assert (np.diff(t[k:]) >= 0).all() and (t[k:] <= 1.0).all()
    # float64 values rounded once
    assert t.size == want.size and (t.view(np.uint32) == want.view(np.uint32)).all()
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.99))
    for step in (1, 2, 10, 100, 1000, t.size - 1, t.size):
        assert t[step - 1] == np.float32(math.sqrt(1.0 - b2 ** step) / (1.0 - b1 ** step))
    # other betas, the degenerate ones included
    for betas in ((0.0, 0.0), (0.5, 0.0), (0.0, 0.5), (0.99, 0.9), (0.9, 0.999)):
        got, exp = runtime.adam_bias_table(*betas), ref.bias_table(*betas)
        assert got.size == exp.size and (got.view(np.uint32) == exp.view(np.uint32)).all(), betas
    # the size query, and a short buffer
    n = C.c_uint32()
    assert lib.nrs_adam_bias_table(0.9, 0.99, None, 0, C.byref(n)) == 0 and n.value == t.size
    short = np.zeros(10, dtype=np.float32)
    assert lib.nrs_adam_bias_table(0.9, 0.99, short.ctypes.data, 10, C.byref(n)) == -1 and "cap" in last_error(lib)
    assert lib.nrs_adam_bias_table(0.9, 0.99, None, 0, None) == -1


def test_bias_table_refuses_betas_too_close_to_one(lib):
    n = C.c_uint32()
    assert lib.nrs_adam_bias_table(0.9, 1.0 - 1e-9, None, 0, C.byref(n)) == -1   # (rounds to 1.0f: outside [0, 1))
    assert lib.nrs_adam_bias_table(0.9, 0.99999, None, 0, C.byref(n)) == -1 and "65536" in last_error(lib)
    assert lib.nrs_adam_bias_table(0.99999, 0.9, None, 0, C.byref(n)) == -1 and "65536" in last_error(lib)
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        assert lib.nrs_adam_bias_table(bad, 0.99, None, 0, C.byref(n)) == -1
        assert lib.nrs_adam_bias_table(0.9, bad, None, 0, C.byref(n)) == -1
    # the largest tables still built: below the limit
    assert lib.nrs_adam_bias_table(0.9, 0.9995, None, 0, C.byref(n)) == 0 and 16384 < n.value <= 65536


def test_exponential_decay_lr(lib):
    from nerfshop_amd import _abi, runtime
    base, start, interval, decay = _abi.BASE_LEARNING_RATE, _abi.BASE_DECAY_START, _abi.BASE_DECAY_INTERVAL, _abi.BASE_DECAY_BASE
    assert (base, start, interval, decay) == (1e-2, 20000, 10000, 0.33)
    d = float(np.float32(0.33))
    b = float(np.float32(1e-2))
    for steps_done, k in ((0, 0), (19999, 0), (20000, 1), (29999, 1), (30000, 2)):
        got = runtime.exponential_decay_lr(steps_done)
        assert np.float32(got) == np.float32(b * d ** k), (steps_done, got)
        assert np.float32(got) == ref.exponential_decay_lr(base, start, interval, decay, steps_done)
    assert runtime.exponential_decay_lr(5, 1.0, 0, 0, 0.5) == 0.5 ** 6   # an interval of 0 counts as 1


# ---- refusals that need no device ------------------------------------------------------------------------------------------------------------------------------
def test_surface_exists(lib):
    import os
    from nerfshop_amd import _abi, runtime, trainer
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nrs.h")).read()
    for name in ("nrs_adam_bias_table", "nrs_exponential_decay_lr", "nrs_optimizer_create", "nrs_optimizer_create_for_model", "nrs_optimizer_destroy",
                 "nrs_optimizer_set_weights", "nrs_optimizer_step", "nrs_optimizer_get_state", "nrs_optimizer_set_state", "nrs_optimizer_export_fp16",
                 "nrs_optimizer_step_count", "nrs_optimizer_set_step_count", "nrs_optimizer_n_params"):
        assert name in _abi.EXPORTS and hasattr(lib, name) and f"{name}(" in header, name
    assert C.sizeof(_abi.AdamParams) == 28 and _abi.AdamParams().struct_size == 28
    for method in ("set_weights", "step", "get_state", "set_state", "export_fp16", "step_count"):
        assert callable(getattr(runtime.Optimizer, method))
    assert callable(trainer.Trainer.step) and callable(trainer.Trainer.update_density_grid)
    assert "Trainer(" in trainer.Trainer.__doc__


def test_create_refusals_before_any_device(lib):
    """nrs_optimizer_create checks its parameters before it looks at the context, so every refusal can be seen without one (the context here is NULL: a call that
    passed all parameter checks ends on that)."""
    from nerfshop_amd import _abi
    out = C.c_void_p()

    def create(n=16, n_matrix=4, p=None, **kw):
        p = _abi.AdamParams(**kw) if p is None else p
        s = lib.nrs_optimizer_create(None, n, n_matrix, C.byref(p), C.byref(out))
        return s, last_error(lib)

    assert create() == (-1, "nrs_optimizer_create: NULL argument")
    for kw, word in ((dict(beta1=1.0), "beta1"), (dict(beta1=-0.5), "beta1"), (dict(beta1=float("nan")), "beta1"), (dict(beta2=1.0), "beta2"),
                     (dict(beta2=-1e-3), "beta2"), (dict(epsilon=-1e-15), "epsilon"), (dict(epsilon=float("inf")), "epsilon"), (dict(l2_reg=-1.0), "l2_reg"),
                     (dict(l2_reg=float("nan")), "l2_reg"), (dict(non_matrix_lr_factor=-1.0), "non_matrix_lr_factor"),
                     (dict(non_matrix_lr_factor=float("inf")), "non_matrix_lr_factor"), (dict(ema_decay=1.0), "ema_decay"), (dict(ema_decay=-0.1), "ema_decay"),
                     (dict(beta2=0.99999), "65536")):
        s, msg = create(**kw)
        assert s == -1 and word in msg, (kw, msg)
    p = _abi.AdamParams()
    p.struct_size -= 4
    s, msg = create(p=p)
    assert s == -1 and "struct_size" in msg
    s, msg = create(n=0, n_matrix=0)
    assert s == -1 and "n_params" in msg
    s, msg = create(n=(1 << 31) + 1)
    assert s == -1 and "n_params" in msg
    s, msg = create(n=16, n_matrix=17)
    assert s == -1 and "n_matrix" in msg
    assert lib.nrs_optimizer_create(None, 16, 4, None, C.byref(out)) == -1 and "params is NULL" in last_error(lib)
    assert lib.nrs_optimizer_create_for_model(None, C.byref(_abi.AdamParams()), C.byref(out)) == -1 and "NULL argument" in last_error(lib)
    assert lib.nrs_optimizer_create_for_model(None, C.byref(_abi.AdamParams(beta1=2.0)), C.byref(out)) == -1 and "beta1" in last_error(lib)
    assert not out.value


def test_null_handles_and_unknown_which(lib):
    buf = np.zeros(4, dtype=np.float32)
    assert lib.nrs_optimizer_set_weights(None, buf.ctypes.data, 0, None) == -1 and "NULL" in last_error(lib)
    assert lib.nrs_optimizer_step(None, None, buf.ctypes.data, 1.0, 1e-2, 0) == -1 and "NULL" in last_error(lib)
    for which in (-1, 6, 99):
        assert lib.nrs_optimizer_get_state(None, which, buf.ctypes.data, 4) == -1 and "unknown `which`" in last_error(lib)
        assert lib.nrs_optimizer_set_state(None, which, buf.ctypes.data, 4) == -1 and "unknown `which`" in last_error(lib)
    assert lib.nrs_optimizer_get_state(None, 0, buf.ctypes.data, 4) == -1 and "NULL" in last_error(lib)
    assert lib.nrs_optimizer_set_state(None, 5, buf.ctypes.data, 4) == -1 and "NULL" in last_error(lib)
    assert lib.nrs_optimizer_export_fp16(None, 2, buf.ctypes.data, None) == -1 and "unknown `which`" in last_error(lib)
    assert lib.nrs_optimizer_export_fp16(None, 0, buf.ctypes.data, None) == -1 and "NULL" in last_error(lib)
    assert lib.nrs_optimizer_set_step_count(None, 3) == -1
    assert lib.nrs_optimizer_step_count(None) == 0 and lib.nrs_optimizer_n_params(None, None) == 0
    lib.nrs_optimizer_destroy(None)  # (a no-op, like free)
