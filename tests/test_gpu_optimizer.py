"""The fused optimiser step on the GPU against the twins of tests/optimizer_ref.py, the optimiser bound to a model, and the Trainer on top of it.

Values (master, m, v, ema) are judged against twin64 in fp32 steps of the exact element; the bar per array is 4 x the worst error of twin32 -- the same operations
in numpy's float32 -- on the same inputs, plus one step (the factor covers a device sqrt and division that differ from numpy's in the last bit); the kernel turned
out bit-equal to twin32 on an MI355X, so that is asserted as well.  Every step is
judged from the state the GPU itself held before it, so the two sides always start from the same numbers.  Counters, skips, the fp16 copy and the gradient's reset
are asserted exactly.  The figures measured on an MI355X are in profiles/optimizer.md."""
import ctypes as C

import numpy as np
import pytest
import torch

import network_backward_ref as nref
import optimizer_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ARRAYS = ("master", "m", "v", "ema")


@pytest.fixture(scope="module")
def ctx(built):
    from nerfshop_amd import runtime
    return runtime.Context(0)


def adam_params(hp):
    from nerfshop_amd import _abi
    return _abi.AdamParams(beta1=hp.beta1, beta2=hp.beta2, epsilon=hp.epsilon, l2_reg=hp.l2_reg, non_matrix_lr_factor=hp.non_matrix_lr_factor, ema_decay=hp.ema_decay)


def make_optimizer(ctx, st, n_matrix, hp):
    """an unbound optimiser holding exactly `st`"""
    from nerfshop_amd import _abi, runtime
    opt = runtime.Optimizer(ctx, n_params=st.master.size, n_matrix=n_matrix, params=adam_params(hp))
    opt.set_weights(st.master)
    for which, a in ((_abi.OPT_M, st.m), (_abi.OPT_V, st.v), (_abi.OPT_STEPS, st.steps), (_abi.OPT_EMA, st.ema), (_abi.OPT_PARAMS_FP16, st.fp16)):
        opt.set_state(which, a)
    opt.set_step_count(st.step_count)
    return opt


def read_state(opt):
    from nerfshop_amd import _abi
    return ref.State(opt.get_state(_abi.OPT_MASTER), opt.get_state(_abi.OPT_M), opt.get_state(_abi.OPT_V), opt.get_state(_abi.OPT_STEPS), opt.get_state(_abi.OPT_EMA),
                     opt.get_state(_abi.OPT_PARAMS_FP16), opt.step_count())


def bits(a):
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same_bits(a, b):
    return all((bits(getattr(a, k)) == bits(getattr(b, k))).all() for k in ("master", "m", "v", "steps", "ema", "fp16")) and a.step_count == b.step_count


SENTINEL = 12345.0


def run_steps(ctx, st, grads, n_matrix, hp, loss_scale, lr, zero_grad, offset):
    """`grads` one after the other through a fresh optimiser; the gradient sits `offset` floats into a larger buffer.  -> the states after each step"""
    opt = make_optimizer(ctx, st, n_matrix, hp)
    n = st.master.size
    buf = torch.full((n + offset + 3,), SENTINEL, dtype=torch.float32, device=DEV)
    view = buf[offset:offset + n]
    assert view.data_ptr() % 16 == (4 * offset) % 16
    states = []
    for g in grads:
        view.copy_(torch.from_numpy(g))
        opt.step(view, loss_scale=loss_scale, lr=lr, zero_grad=zero_grad)
        states.append(read_state(opt))
        after = buf.cpu().numpy()
        assert (after[:offset] == SENTINEL).all() and (after[offset + n:] == SENTINEL).all(), "a write outside the gradient"
        if zero_grad:
            assert (bits(after[offset:offset + n]) == 0).all(), "zero_grad leaves the gradient all zero"
        else:
            assert (bits(after[offset:offset + n]) == bits(g)).all(), "without zero_grad the gradient is untouched"
    opt.close()
    return states


def judge_step(before, after, g, n_matrix, hp, loss_scale, lr, table, worst):
    """exact assertions and the value bar for one step; `worst` collects (gpu, twin32) per array"""
    t64 = ref.twin64(before, g, hp, n_matrix, loss_scale, lr, table, fp16_for_ema=after.fp16)
    t32 = ref.twin32(before, g, hp, n_matrix, loss_scale, lr, table)
    t32_ema_exact = ref.twin64(before, g, hp, n_matrix, loss_scale, lr, table, fp16_for_ema=t32.fp16).ema
    assert (after.steps == t64.steps).all() and after.step_count == t64.step_count
    skipped = after.steps == before.steps
    assert (skipped == ((np.arange(g.size) >= n_matrix) & (g == 0))).all()
    for k in ("master", "m", "v", "fp16"):
        assert (bits(getattr(after, k))[skipped] == bits(getattr(before, k))[skipped]).all(), f"skipped elements keep {k} bit for bit"
    with np.errstate(over="ignore"):
        assert (bits(after.fp16)[~skipped] == bits(after.master.astype(np.float16))[~skipped]).all(), "fp16 is the rounding of the stored master weight"
    equal = True
    for k in ARRAYS:
        e_gpu = float(ref.ulp_error(getattr(after, k), getattr(t64, k)).max())
        e_32 = float(ref.ulp_error(getattr(t32, k), t32_ema_exact if k == "ema" else getattr(t64, k)).max())
        worst[k] = (max(worst[k][0], e_gpu), max(worst[k][1], e_32))
        assert e_gpu <= 4.0 * e_32 + 1.0, (k, e_gpu, e_32)
    # Measured on an MI355X: the kernel is bit-equal to twin32 (IEEE division and square root, no contraction, the same order), which implies the bar above.  So that
    # is asserted: master, m, v and the stored fp16 against twin32, and the EMA against twin32's multiply-add on the same fp16.
    for k in ("master", "m", "v", "fp16", "ema"):
        assert (bits(getattr(after, k)) == bits(getattr(t32, k))).all(), f"{k} is bit-equal to the float32 twin"
    return True


SHAPES = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4099)


@pytest.mark.parametrize("n", SHAPES)
def test_shapes_against_the_twins(ctx, n):
    """Every n with every n_matrix of {0, 1, 2, 5, n - 1, n} that fits: three steps with changing zero patterns (half of the non-matrix gradients exactly zero, in
    runs and singly inside a group of four, one of them -0.0) from a gradient one float off 16-byte alignment, with zero_grad; the same run again (bit-identical);
    and once more from an aligned gradient without zero_grad (bit-identical state, gradient untouched)."""
    hp = ref.Hyper(non_matrix_lr_factor=0.5)
    table = ref.bias_table(hp.beta1, hp.beta2)
    loss_scale, lr = 128.0, 1e-2
    worst = {k: (0.0, 0.0) for k in ARRAYS}
    all_equal = True
    for n_matrix in sorted({k for k in (0, 1, 2, 5, n - 1, n) if 0 <= k <= n}):
        rng = np.random.default_rng(1000 * n + n_matrix)
        st = ref.random_state(rng, n, n_matrix)
        grads = [ref.random_grad(rng, n, n_matrix, loss_scale) for _ in range(3)]
        if n - n_matrix >= 50:
            assert all(0.3 < (g[n_matrix:] == 0).mean() < 0.7 for g in grads) and all(np.signbit(g[g == 0]).any() for g in grads)
        states = run_steps(ctx, st, grads, n_matrix, hp, loss_scale, lr, zero_grad=True, offset=1)
        before = st
        for g, after in zip(grads, states):
            all_equal &= judge_step(before, after, g, n_matrix, hp, loss_scale, lr, table, worst)
            before = after
        if n - n_matrix >= 8:
            assert len(set(states[-1].steps[n_matrix:].tolist())) > 1, "the step counts of neighbours diverge"
        again = run_steps(ctx, st, grads, n_matrix, hp, loss_scale, lr, zero_grad=True, offset=1)
        aligned = run_steps(ctx, st, grads, n_matrix, hp, loss_scale, lr, zero_grad=False, offset=0)
        for a, b, c in zip(states, again, aligned):
            assert same_bits(a, b), "two identical runs are bit-identical"
            assert same_bits(a, c), "alignment and zero_grad do not change the state"
    print(f"n={n}: worst error in fp32 ulps, GPU / twin32: " + "  ".join(f"{k} {worst[k][0]:.2f} / {worst[k][1]:.2f}" for k in ARRAYS) +
          f"   master, m, v bit-equal to twin32: {all_equal}")


def test_a_table_too_long_for_lds(ctx):
    """beta2 = 0.999: 16 628 table entries, more than the step stages in LDS, so it reads the table through L2 -- the same assertions"""
    hp = ref.Hyper(beta2=0.999)
    table = ref.bias_table(hp.beta1, hp.beta2)
    assert table.size > 4096
    n, n_matrix = 257, 5
    rng = np.random.default_rng(77)
    st = ref.random_state(rng, n, n_matrix, steps_max=20000)
    grads = [ref.random_grad(rng, n, n_matrix, 128.0) for _ in range(2)]
    worst = {k: (0.0, 0.0) for k in ARRAYS}
    before = st
    for g, after in zip(grads, run_steps(ctx, st, grads, n_matrix, hp, 128.0, 1e-2, zero_grad=True, offset=1)):
        judge_step(before, after, g, n_matrix, hp, 128.0, 1e-2, table, worst)
        before = after


def test_beyond_the_table(ctx):
    """steps preset to T_sat - 1, T_sat and T_sat + 5: the step that follows reads a factor of exactly 1 in all three, so elements that differ in nothing else end
    bit-identical; the counters go on counting."""
    hp = ref.Hyper(ema_decay=0.0)
    table = ref.bias_table(hp.beta1, hp.beta2)
    T = table.size
    assert table[T - 1] == 1.0 and table[T - 2] != 1.0
    n, n_matrix = 24, 3   # 8 triples: elements 3k, 3k+1, 3k+2 share everything but the counter
    rng = np.random.default_rng(9)
    triple = lambda a: np.repeat(a[:8], 3)
    base = ref.random_state(rng, n, 0)
    st = ref.State(triple(base.master), triple(base.m), triple(base.v), np.tile(np.array([T - 1, T, T + 5], dtype=np.uint32), 8), triple(base.ema),
                   triple(base.master).astype(np.float16), T + 5)
    g = triple(ref.random_grad(rng, n, 0, 128.0, zero_share=0.0))
    after, = run_steps(ctx, st, [g], n_matrix, hp, 128.0, 1e-2, zero_grad=True, offset=0)
    assert (after.steps == st.steps + 1).all()
    for k in ("master", "m", "v", "fp16"):
        a = bits(getattr(after, k)).reshape(8, 3)[1:]   # (the first triple straddles the matrix boundary: L2 applies to its elements)
        assert (a[:, 0] == a[:, 1]).all() and (a[:, 1] == a[:, 2]).all(), k
    worst = {k: (0.0, 0.0) for k in ARRAYS}
    judge_step(st, after, g, n_matrix, hp, 128.0, 1e-2, table, worst)
    # one step earlier the factor is the table's last value below 1: the twin reads table[T_sat - 2] there, and the bar holds as well
    st.steps[:] = T - 2
    after, = run_steps(ctx, st, [g], n_matrix, hp, 128.0, 1e-2, zero_grad=True, offset=0)
    judge_step(st, after, g, n_matrix, hp, 128.0, 1e-2, table, worst)


def test_l2_boundary_inside_a_vector(ctx):
    """zero gradient everywhere, l2_reg = 0.5, the matrix / non-matrix boundary in the middle of a group of four: matrix weights move by the twin's amount, the
    others not at all"""
    hp = ref.Hyper(l2_reg=0.5, ema_decay=0.0)
    table = ref.bias_table(hp.beta1, hp.beta2)
    n, n_matrix = 16, 6
    st = ref.random_state(np.random.default_rng(4), n, n_matrix)
    g = np.zeros(n, dtype=np.float32)
    after, = run_steps(ctx, st, [g], n_matrix, hp, 128.0, 1e-2, zero_grad=True, offset=1)
    worst = {k: (0.0, 0.0) for k in ARRAYS}
    judge_step(st, after, g, n_matrix, hp, 128.0, 1e-2, table, worst)
    assert (after.master[:n_matrix] != st.master[:n_matrix]).all() and (after.steps[:n_matrix] == st.steps[:n_matrix] + 1).all()
    for k in ("master", "m", "v", "steps", "fp16", "ema"):
        assert (bits(getattr(after, k))[n_matrix:] == bits(getattr(st, k))[n_matrix:]).all(), k


def test_ema(ctx):
    """three steps with ema_decay = 0.95 against the twin, the elements the Adam part skipped included; ema_decay = 0 leaves the ema array untouched"""
    n, n_matrix = 257, 5
    rng = np.random.default_rng(12)
    st = ref.random_state(rng, n, n_matrix)
    st.step_count = 0
    grads = [ref.random_grad(rng, n, n_matrix, 128.0) for _ in range(3)]
    hp = ref.Hyper()
    table = ref.bias_table(hp.beta1, hp.beta2)
    states = run_steps(ctx, st, grads, n_matrix, hp, 128.0, 1e-2, zero_grad=True, offset=1)
    worst = {k: (0.0, 0.0) for k in ARRAYS}
    before = st
    for g, after in zip(grads, states):
        judge_step(before, after, g, n_matrix, hp, 128.0, 1e-2, table, worst)
        skipped = after.steps == before.steps
        assert skipped.sum() > 50
        if before is st:
            # step 1 (a = 0, b = 1) replaces the initial value by the stored fp16, skipped or not.  Later steps are judged by the twin alone: where Adam skips twice
            # running, a ema + b fp16 with a + b = 1 and ema == fp16 gives the same value again, as it should.
            assert (after.ema[skipped] != before.ema[skipped]).mean() > 0.9, "the EMA moves where Adam skipped"
        before = after
    # step 1 of a fresh optimiser forgets the initial value: a = 0, b = 1
    assert (states[0].ema == states[0].fp16.astype(np.float32)).all()
    print("ema: worst error in fp32 ulps, GPU / twin32:", "%.2f / %.2f" % worst["ema"])
    hp0 = ref.Hyper(ema_decay=0.0)
    st.ema = np.arange(n, dtype=np.float32) + 0.5
    for after in run_steps(ctx, st, grads, n_matrix, hp0, 128.0, 1e-2, zero_grad=False, offset=0):
        assert (bits(after.ema) == bits(st.ema)).all()


def test_step_refusals(ctx):
    from nerfshop_amd import _abi, runtime
    opt = runtime.Optimizer(ctx, n_params=8, n_matrix=2)
    g = torch.zeros(8, dtype=torch.float32, device=DEV)
    with pytest.raises(runtime.NrsError, match="nrs error -5.*weights not set"):
        opt.step(g)
    with pytest.raises(runtime.NrsError, match="nrs error -5"):
        opt.get_state(_abi.OPT_MASTER)
    with pytest.raises(runtime.NrsError, match="nrs error -5"):
        opt.export_fp16()
    opt.set_weights(np.ones(8, dtype=np.float32))
    for kw, word in ((dict(loss_scale=0.0), "loss_scale"), (dict(loss_scale=-1.0), "loss_scale"), (dict(loss_scale=float("inf")), "loss_scale"),
                     (dict(loss_scale=float("nan")), "loss_scale"), (dict(lr=-1e-2), "learning_rate"), (dict(lr=float("nan")), "learning_rate")):
        with pytest.raises(runtime.NrsError, match="nrs error -1.*" + word):
            opt.step(g, **kw)
    assert opt.lib.nrs_optimizer_step(opt.h, None, None, 1.0, 1e-2, 0) == -1
    out = np.zeros(9, dtype=np.float32)
    assert opt.lib.nrs_optimizer_get_state(opt.h, _abi.OPT_M, out.ctypes.data, 9) == -1 and "n_params" in opt.lib.nrs_last_error().decode()
    assert opt.lib.nrs_optimizer_set_state(opt.h, _abi.OPT_M, out.ctypes.data, 7) == -1
    assert opt.lib.nrs_optimizer_get_state(opt.h, 6, out.ctypes.data, 8) == -1 and "unknown" in opt.lib.nrs_last_error().decode()
    assert opt.step_count() == 0 and (opt.get_state(_abi.OPT_STEPS) == 0).all(), "a refused step changes nothing"
    opt.step(g, lr=0.0)   # a learning rate of 0 is a step like any other
    assert opt.step_count() == 1
    opt.close()


# ---- bound to a model ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def desc14():
    from nerfshop_amd import synth
    return synth.model_desc(log2_hashmap_size=14)


@pytest.mark.parametrize("cell_cache_bytes", [0, 4 << 20])
def test_bound_model_reads_what_the_optimiser_wrote(ctx, desc14, cell_cache_bytes):
    """After set_weights and after a step, inference on 777 fixed inputs through the bound model is bit-identical to a second model that received
    export_fp16(WEIGHTS) through set_params_device -- without records and with a cell cache of at least two levels on the bound model."""
    from nerfshop_amd import _abi, runtime
    bound = runtime.NerfNetwork(ctx, desc14, cell_cache_bytes=0)
    if cell_cache_bytes:
        bound.set_cell_cache(cell_cache_bytes)
        n_levels = C.c_uint32()
        assert bound.lib.nrs_model_cell_cache_bytes(bound.h, C.byref(n_levels)) > 0 and n_levels.value >= 2
    other = runtime.NerfNetwork(ctx, desc14, cell_cache_bytes=0)
    opt = runtime.Optimizer(ctx, network=bound)
    n = bound.n_params()
    assert (opt.n_params, opt.n_matrix) == (n, nref.N_MLP)
    weights = nref.make_params(desc14, 11).astype(np.float32)
    rng = np.random.default_rng(31)
    weights += (rng.normal(size=n) * 1e-5).astype(np.float32)   # off the fp16 lattice: the rounding is the optimiser's
    coords = torch.from_numpy(nref.make_coords(np.random.default_rng(5), 777)).to(DEV)

    def both():
        outs = []
        other.set_params_device(opt.export_fp16(_abi.OPT_EXPORT_WEIGHTS))
        for net in (bound, other):
            o = torch.zeros((777, 16), dtype=torch.float16, device=DEV)
            net.inference_mixed_precision(None, coords, o)
            outs.append(o.cpu().numpy().view(np.uint16))
        return outs

    opt.set_weights(torch.from_numpy(weights).to(DEV))
    a, b = both()
    assert (a == b).all() and a.any()
    with np.errstate(over="ignore"):
        assert (bits(opt.get_state(_abi.OPT_PARAMS_FP16)) == bits(weights.astype(np.float16))).all()
    first = a.copy()
    grad = torch.from_numpy(ref.random_grad(rng, n, nref.N_MLP, 128.0, zero_share=0.9)).to(DEV)
    opt.step(grad, loss_scale=128.0, lr=1e-2, zero_grad=True)
    a, b = both()
    assert (a == b).all() and (a != first).any(), "the bound model reads the stepped parameters"
    assert float(grad.abs().max()) == 0
    fp16 = opt.get_state(_abi.OPT_PARAMS_FP16)
    with np.errstate(over="ignore"):
        assert (bits(fp16) == bits(opt.get_state(_abi.OPT_MASTER).astype(np.float16))).all()
    assert (bits(opt.export_fp16(_abi.OPT_EXPORT_WEIGHTS).cpu().numpy()) == bits(fp16)).all()
    # the EMA blob: get_state(EMA) rounded
    with np.errstate(over="ignore"):
        want = opt.get_state(_abi.OPT_EMA).astype(np.float16)
    assert (bits(opt.export_fp16(_abi.OPT_EXPORT_EMA).cpu().numpy()) == bits(want)).all()
    opt.close(); bound.close(); other.close()


def test_fit_through_backward_and_the_fused_step(ctx, desc14):
    """The student / teacher case of test_gpu_network_backward.py (seeds 11 and 7, 4 096 samples, 20 steps, lr 1e-2, eps 1e-15) through backward(accumulate=True) and
    Optimizer.step(zero_grad=True).  r_ref: the same loop on the CPU, network_backward_ref's forward with twin64 as the optimiser."""
    from nerfshop_amd import runtime
    hp = ref.Hyper()
    table = ref.bias_table(hp.beta1, hp.beta2)
    lt = nref.level_table(desc14)
    coords = nref.make_coords(np.random.default_rng(8), 4096)
    teacher, student = nref.make_params(desc14, 7), nref.make_params(desc14, 11)
    target = nref.forward(lt, torch.from_numpy(teacher.astype(np.float64)), coords).detach()[:, :4]
    n = student.size
    z = lambda dt=np.float32: np.zeros(n, dtype=dt)
    st = ref.State(student.astype(np.float32), z(), z(), z(np.uint32), student.astype(np.float32), student.astype(np.float16), 0)
    ref_losses = []
    for step in range(21):
        p = torch.from_numpy(st.fp16.astype(np.float64)).requires_grad_(True)
        loss = ((nref.forward(lt, p, coords)[:, :4] - target) ** 2).mean()
        ref_losses.append(loss.item())
        if step == 20:
            break
        gp, = torch.autograd.grad(loss, p)
        st = ref.twin64(st, gp.numpy(), hp, nref.N_MLP, 1.0, 1e-2, table)
        st.master, st.m, st.v, st.ema = (a.astype(np.float32) for a in (st.master, st.m, st.v, st.ema))
    r_ref = ref_losses[-1] / ref_losses[0]

    net = runtime.NerfNetwork(ctx, desc14, cell_cache_bytes=0)
    opt = runtime.Optimizer(ctx, network=net, params=adam_params(hp))
    opt.set_weights(student.astype(np.float32))
    x, y = torch.from_numpy(coords).to(DEV), target.to(torch.float32).to(DEV)
    out = torch.zeros((4096, 16), dtype=torch.float16, device=DEV)
    dl = torch.zeros((4096, 16), dtype=torch.float16, device=DEV)
    grad = torch.zeros(n, dtype=torch.float32, device=DEV)
    losses = []
    for step in range(21):
        net.inference_mixed_precision(None, x, out)
        diff = out[:, :4].to(torch.float32) - y
        losses.append(float((diff ** 2).mean()))
        if step == 20:
            break
        dl[:, :4] = (diff * (2.0 / diff.numel() * nref.LOSS_SCALE)).to(torch.float16)
        net.backward(None, x, dl, grad, None, accumulate=True)
        opt.step(grad, loss_scale=nref.LOSS_SCALE, lr=1e-2, zero_grad=True)
    r = losses[-1] / losses[0]
    print(f"fit: reference loss {ref_losses[0]:.5f} -> {ref_losses[-1]:.5f} (ratio {r_ref:.4f}); GPU loss {losses[0]:.5f} -> {losses[-1]:.5f} (ratio {r:.4f})")
    assert abs(losses[0] - ref_losses[0]) <= 1e-3 * ref_losses[0]
    assert r <= r_ref + 0.1 * (1.0 - r_ref)
    assert float(grad.abs().max()) == 0 and opt.step_count() == 20, "the gradient buffer is all zero after the last step"
    opt.close(); net.close()


# ---- the Trainer -----------------------------------------------------------------------------------------------------------------------------------------------
def pinhole_rays(camera, width, height, camera_angle_x):
    """origin and unit direction per pixel centre of a camera given as synth.orbit_camera's column-major 3 x 4 matrix"""
    cam = np.asarray(camera, np.float64).reshape(4, 3).T   # columns: three axes, origin
    focal = 0.5 * width / np.tan(0.5 * camera_angle_x)
    xs, ys = np.meshgrid(np.arange(width) + 0.5, np.arange(height) + 0.5)
    d = np.stack([(xs - 0.5 * width) / focal, (ys - 0.5 * height) / focal, np.ones_like(xs)], -1).reshape(-1, 3) @ cam[:, :3].T
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([np.broadcast_to(cam[:, 3], d.shape), d], 1).astype(np.float32)


def test_trainer(ctx, desc14):
    """256 rays of an orbit camera, targets from a teacher model's render of the same view, 10 steps with one update_density_grid(): the loss falls, and step()
    returns while the device is still busy with work enqueued before it (it never waits)."""
    from nerfshop_amd import runtime, synth
    from nerfshop_amd.trainer import Trainer
    W = H = 16
    camera = synth.orbit_camera(30.0)
    tb = runtime.Testbed(ctx, desc14, 1)
    tb.nerf_network.set_params(synth.make_params(desc14))
    grid = synth.density_grid(1)
    tb.nerf_network.set_density_grid(grid)
    p = synth.render_params(W, H, camera)
    p.linear_colors = 1
    buf = runtime.RenderBuffer(W, H)
    buf.clear_frame()
    tb.render_with_params(tb.nerf_network, p, buf.frame_buffer(), buf.depth_buffer())
    target = buf.frame_buffer().reshape(-1, 4).clone()
    assert float(target[:, 3].max()) > 0.5, "the teacher's view shows the scene"
    rays = torch.from_numpy(pinhole_rays(camera, W, H, synth.CAMERA_ANGLE_X)).to(DEV)

    trainer = Trainer(ctx, desc14, seed=11, density_grid=grid, max_samples=1 << 17)
    assert trainer.grad.numel() == trainer.network.n_params() and trainer.current_learning_rate() == pytest.approx(1e-2)
    losses = []
    busy = torch.randn(8192, 8192, device=DEV)
    stream = torch.cuda.current_stream()
    for step in range(10):
        if step == 5:
            trainer.update_density_grid()
        if step == 7:   # every buffer exists by now: a step allocates nothing
            torch.cuda.synchronize()
            for _ in range(6):
                busy = (busy @ busy) * 1e-4   # some tens of milliseconds of work ahead of the step
            losses.append(trainer.step(rays, target))
            assert not stream.query(), "Trainer.step returned with the stream drained: it has waited for the device"
        else:
            losses.append(trainer.step(rays, target))
    torch.cuda.synchronize()
    losses = [float(v) for v in losses]
    print("trainer losses:", " ".join(f"{v:.5f}" for v in losses))
    assert all(np.isfinite(losses)) and losses[0] > 0
    assert np.mean(losses[-3:]) < np.mean(losses[:3])
    assert trainer.training_step == 10 and trainer.optimizer.step_count() == 10
    assert float(trainer.grad.abs().max()) == 0, "the persistent gradient buffer is zero between steps"
