"""nrs_network_backward on the GPU against the float64 twin of tests/network_backward_ref.py.

Metric: relative L2 error per block -- each of the five matrices, each of the sixteen grid levels -- against the twin's EXACT gradient (round_back off).
Bars: 8 x 2^-11 for n >= 63 (five gradient roundings on the longest chain, the scaled dL_doutput cast, the forward's rare one-ulp differences: each at most one
unit relative), 16 x 2^-11 for n = 1 (nothing averages inside a block; the rounding twin alone reaches 4.7 units there), and at n = 777 additionally 4 x the
gap between the rounding twin and the exact one on the same inputs.  All at log2_hashmap_size 14.
"""
import ctypes as C

import numpy as np
import pytest

import network_backward_ref as ref

pytestmark = pytest.mark.gpu

UNIT = 2.0 ** -11
INVALID, UNSUPPORTED = -1, -2


class Rig:
    def __init__(self):
        import torch
        from nerfshop_amd import runtime, synth
        self.torch, self.rt, self.synth = torch, runtime, synth
        self.desc = synth.model_desc(1, log2_hashmap_size=14)
        self.lt = ref.level_table(self.desc)
        self.p16 = ref.make_params(self.desc, 7)
        self.ctx = runtime.Context(0)
        self.net = runtime.NerfNetwork(self.ctx, self.desc, cell_cache_bytes=0)
        self.net.set_params(self.p16)
        self.n_params = self.net.n_params()
        # the shared 777-sample case: inputs, dL_doutput, both twins (computed once, never modified)
        rng = np.random.default_rng(100)
        self.coords = ref.make_coords(rng, 777)
        self.dl = make_dl(rng, 777)
        self.exact = ref.gradient(self.lt, self.p16, self.coords, self.dl)
        self.rounded = ref.gradient(self.lt, self.p16, self.coords, self.dl, round_back=True)
        self.gap = ref.block_errors(self.lt, self.rounded, self.exact)

    def scaled_fp16(self, dl, layout):
        t = self.torch.from_numpy((np.asarray(dl, np.float32) * np.float32(ref.LOSS_SCALE)).astype(np.float16))
        return (t.T.contiguous() if layout == "planes" else t.contiguous()).cuda()

    def backward(self, coords, dl, layout="interleaved", accumulate=False, out=None, want_input=False, raw_dl=None):
        torch = self.torch
        cin = torch.from_numpy(np.ascontiguousarray(coords, np.float32)).cuda()
        dl16 = raw_dl if raw_dl is not None else self.scaled_fp16(dl, layout)
        if out is None:
            out = torch.full((self.n_params,), float("nan"), dtype=torch.float32, device="cuda:0")  # accumulate = False must overwrite it
        din = torch.full(cin.shape, float("nan"), dtype=torch.float32, device="cuda:0") if want_input else None
        self.net.backward(None, cin, dl16, out, din, accumulate=accumulate)
        torch.cuda.synchronize()
        g = out.cpu().numpy().astype(np.float64) / ref.LOSS_SCALE
        return (g, din.cpu().numpy()) if want_input else g


def make_dl(rng, n):
    dl = np.zeros((n, 16), np.float32)
    dl[:, :4] = rng.normal(size=(n, 4)).astype(np.float16).astype(np.float32) / n
    return dl


@pytest.fixture(scope="module")
def rig(built):
    return Rig()


def check_blocks(rig, got, want, bar, gap=None, what=""):
    assert np.isfinite(got).all(), "non-finite gradient"
    errs = ref.block_errors(rig.lt, got, want)
    for name, e in errs.items():
        print(f"{what} {name:4s} rel L2 {e:.3e} = {e / UNIT:.2f} units" + (f"   twin gap {gap[name]:.3e}" if gap else ""))
    worst = max(errs, key=errs.get)
    print(f"{what} worst block {worst}: {errs[worst]:.3e} (bar {bar:.3e})")
    for name, e in errs.items():
        assert e <= bar, (name, e, bar)
        if gap is not None:
            assert e <= 4.0 * gap[name], (name, e, gap[name])
    assert (got[9216 + 3 * 64:ref.N_MLP] == 0).all(), "rows 3..15 of the rgb output matrix"
    return errs


@pytest.mark.parametrize("n,layout", [(1, "interleaved"), (63, "interleaved"), (64, "planes"), (65, "interleaved"), (777, "interleaved"), (777, "planes")])
def test_gradient_against_twin(rig, n, layout):
    if n == 777:
        coords, dl, want, gap = rig.coords, rig.dl, rig.exact, rig.gap
    else:
        rng = np.random.default_rng(200 + n)
        coords, dl = ref.make_coords(rng, n), make_dl(rng, n)
        want, gap = ref.gradient(rig.lt, rig.p16, coords, dl), None
    got = rig.backward(coords, dl, layout)
    check_blocks(rig, got, want, (16 if n == 1 else 8) * UNIT, gap, f"n={n} {layout}")


def test_padding_rows_are_never_read(rig):
    rng = np.random.default_rng(265)
    coords, dl = ref.make_coords(rng, 65), make_dl(rng, 65)
    want = ref.gradient(rig.lt, rig.p16, coords, dl)
    poisoned = dl.copy()
    poisoned[:, 4:] = np.nan
    check_blocks(rig, rig.backward(coords, poisoned), want, 8 * UNIT, None, "NaN rows 4..15")


def test_many_samples_on_the_same_entries(rig):
    coords = rig.coords.copy()
    coords[:64, :3] = coords[0, :3]
    want = ref.gradient(rig.lt, rig.p16, coords, rig.dl)
    check_blocks(rig, rig.backward(coords, rig.dl), want, 8 * UNIT, None, "64 samples at one position")


def test_more_tiles_than_resident_waves(rig):
    """The 777-sample batch 600 times: 7285 tiles, several per wave of any launch shape (one 4-wave workgroup per CU: 1024 waves); linear in the batch."""
    reps = 600
    assert (777 * reps + 63) // 64 > 4 * 4 * rig.ctx.n_cus
    got = rig.backward(np.tile(rig.coords, (reps, 1)), np.tile(rig.dl, (reps, 1)))
    check_blocks(rig, got, reps * rig.exact, 8 * UNIT, None, f"{reps} x 777")


def test_accumulate(rig):
    torch = rig.torch
    buf = torch.full((rig.n_params,), float("nan"), dtype=torch.float32, device="cuda:0")
    once = rig.backward(rig.coords, rig.dl, out=buf, accumulate=False)  # overwrites the NaNs
    assert np.isfinite(once).all()
    check_blocks(rig, once, rig.exact, 8 * UNIT, None, "overwrite")
    rig.backward(rig.coords, rig.dl, out=buf, accumulate=True)
    thrice = rig.backward(rig.coords, rig.dl, out=buf, accumulate=True)
    for name, a, b in ref.blocks(rig.lt):
        rel = np.linalg.norm(thrice[a:b] - 3 * once[a:b]) / np.linalg.norm(3 * once[a:b])
        assert rel <= 1e-5, (name, rel)
    # n = 0: nothing launched, the buffer still zeroed
    empty = torch.zeros((0, 7), dtype=torch.float32, device="cuda:0")
    rig.net.backward(None, empty, torch.zeros((0, 16), dtype=torch.float16, device="cuda:0"), buf, None, accumulate=False)
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0


def test_refusals(rig):
    from nerfshop_amd import _abi
    torch, rt, synth = rig.torch, rig.rt, rig.synth
    lib = rig.ctx.lib
    cin = torch.zeros((64, 10), dtype=torch.float32, device="cuda:0")
    dl = torch.zeros((64, 16), dtype=torch.float16, device="cuda:0")

    def call(net, n_params, ld_in=7):
        out = torch.zeros(max(int(n_params), 1), dtype=torch.float32, device="cuda:0")
        return lib.nrs_network_backward(net.h, None, 64, cin.data_ptr(), ld_in, dl.data_ptr(), 16, _abi.LAYOUT_INTERLEAVED, out.data_ptr(), int(n_params), 0, None)

    others = {
        "rgb_hidden_layers": rt.NerfNetwork(rig.ctx, synth.model_desc(1, rgb_hidden_layers=1, log2_hashmap_size=14), cell_cache_bytes=0),
        "sh_degree": rt.NerfNetwork(rig.ctx, synth.model_desc(1, no_dir=True, log2_hashmap_size=14), cell_cache_bytes=0),
        "n_extra_dims": rt.NerfNetwork(rig.ctx, rig.desc, cell_cache_bytes=0, n_extra_dims=3),
    }
    for field, net in others.items():
        assert call(net, net.n_params(), 10) == UNSUPPORTED, field
        assert field.encode() in lib.nrs_last_error(), lib.nrs_last_error()
    twin = rt.NerfNetwork(rig.ctx, rig.desc, cell_cache_bytes=0)
    twin.set_params(rig.p16)
    twin.set_numerics(1, 1)
    assert call(twin, twin.n_params()) == UNSUPPORTED
    assert b"numerics" in lib.nrs_last_error()
    twin.set_numerics(0, 0)
    assert call(twin, twin.n_params()) == 0
    assert call(twin, twin.n_params() - 1) == INVALID
    assert b"n_params" in lib.nrs_last_error()
    fresh = rt.NerfNetwork(rig.ctx, rig.desc, cell_cache_bytes=0)
    assert call(fresh, fresh.n_params()) == -5  # NRS_ERR_STATE: parameters not set
    torch.cuda.synchronize()


def test_input_gradient_of_the_density(rig):
    """row 3 = 128, all else zero: the chain of nrs_network_input_gradient (same fragments, same roundings)"""
    torch = rig.torch
    raw = torch.zeros((777, 16), dtype=torch.float16, device="cuda:0")
    raw[:, 3] = 128.0
    _, din = rig.backward(rig.coords, None, want_input=True, raw_dl=raw)
    want = torch.empty((777, 3), dtype=torch.float32, device="cuda:0")
    rig.net.input_gradient(None, torch.from_numpy(rig.coords).cuda(), want)
    torch.cuda.synchronize()
    want = want.cpu().numpy().astype(np.float64)
    got = din[:, :3].astype(np.float64) / 128.0
    assert np.linalg.norm(got - want) <= 1e-6 * np.linalg.norm(want)
    assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()
    assert (din[:, 3:] == 0).all()


def test_input_gradient_against_twin(rig):
    rng = np.random.default_rng(307)
    coords = ref.make_coords(rng, 777, margin=1e-3, lt=rig.lt)
    dl = make_dl(rng, 777)
    want_p, want_x = ref.gradient(rig.lt, rig.p16, coords, dl, want_input=True)
    got_p, din = rig.backward(coords, dl, want_input=True)
    check_blocks(rig, got_p, want_p, 8 * UNIT, None, "with dL_dinput")
    got_x = din[:, :3].astype(np.float64) / ref.LOSS_SCALE
    err = np.linalg.norm(got_x - want_x) / np.linalg.norm(want_x)
    print(f"dL/dposition rel L2 {err:.3e} = {err / UNIT:.2f} units")
    assert err <= 8 * UNIT
    assert (din[:, 3:] == 0).all()


def test_fit_through_the_torch_module(rig):
    """Student (seed 11) learns the teacher's (seed 7) channels 0..3 at 4096 fixed samples, Adam(1e-2, eps 1e-15), 20 steps: at least nine tenths of the loss reduction
    the same loop reaches on the CPU with the twin (fp32 master, fp16 parameters in the forward)."""
    torch = rig.torch
    from nerfshop_amd.torch_module import NerfNetworkModule
    coords = ref.make_coords(np.random.default_rng(8), 4096)
    teacher, student = ref.make_params(rig.desc, 7), ref.make_params(rig.desc, 11)
    ref_losses, target = ref.fit_loop(rig.lt, teacher, student, coords, steps=20)
    r_ref = ref_losses[-1] / ref_losses[0]

    net = NerfNetworkModule(rig.desc, params_fp16=student, ctx=rig.ctx)
    assert [tuple(p.shape) for p in net.parameters()] == [(rig.n_params,)] and net.params.dtype == torch.float32
    opt = torch.optim.Adam(net.parameters(), lr=1e-2, eps=1e-15)
    x = torch.from_numpy(coords).cuda()
    y = target.to(torch.float32).cuda()
    losses = []
    for step in range(21):
        loss = ((net(x)[:, :4] - y) ** 2).mean()
        losses.append(float(loss.detach()))
        if step == 20:
            break
        opt.zero_grad()
        loss.backward()
        opt.step()
    r = losses[-1] / losses[0]
    print(f"fit: reference loss {ref_losses[0]:.5f} -> {ref_losses[-1]:.5f} (ratio {r_ref:.4f}); GPU loss {losses[0]:.5f} -> {losses[-1]:.5f} (ratio {r:.4f})")
    assert abs(losses[0] - ref_losses[0]) <= 1e-3 * ref_losses[0]
    assert r <= r_ref + 0.1 * (1.0 - r_ref)
