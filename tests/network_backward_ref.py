"""The yardstick of the backward-pass tests: an independent twin of base.json's NerfNetwork in torch on the CPU, float64, differentiated by autograd.

Written from the description of the network (include/nrs.h), not from the kernels: the level table comes from the oracle (orc_model_level_table), cell
indices and trilinear weights are computed in float32 the way the oracle's hashgrid_encode_one does (its fmaf included), everything after them is float64 matrix algebra.  Every fp16
rounding point of the forward pass is straight-through, x + (round_fp16(x) - x).detach(): the forward values are the network's fp16 values, the derivative is the
derivative of the unrounded network at those values.  `round_back` additionally rounds the GRADIENT to fp16 where the fully fused backward pass does (one rounding
per layer boundary): an identity whose backward rounds.  Rows 4..15 of the output take no gradient (extract_rgb copies three rows).
"""
import ctypes as C
import math

import numpy as np
import torch

from oracle import oracle as orc

N_MLP = 10240
# name, first parameter, one past the last: the five matrices in the blob's order
MATRICES = [("dW1", 0, 2048), ("dW2", 2048, 3072), ("rW1", 3072, 5120), ("rW2", 5120, 9216), ("rW3", 9216, 10240)]
LOSS_SCALE = 128.0


def level_table(desc):
    lib = orc.load()
    scale = np.zeros(16, np.float32)
    res, off, cnt, hashed = (np.zeros(16, np.uint32) for _ in range(4))
    lib.orc_model_level_table(C.byref(desc), scale.ctypes.data, res.ctypes.data, off.ctypes.data, cnt.ctypes.data, hashed.ctypes.data)
    return scale, res, off, cnt, hashed


def n_params(desc):
    return int(orc.load().orc_model_n_params(C.byref(desc)))


def blocks(lt):
    """the blocks the error metric is taken over: five matrices, sixteen grid levels"""
    b = list(MATRICES)
    for l in range(16):
        b.append(("L%d" % l, N_MLP + 2 * int(lt[2][l]), N_MLP + 2 * (int(lt[2][l]) + int(lt[3][l]))))
    return b


def make_params(desc, seed, grid_range=0.5):
    """Xavier-uniform matrices and a U(-grid_range, grid_range) grid from numpy's PCG64 -> fp16 blob"""
    rng = np.random.Generator(np.random.PCG64(seed))

    def xavier(o, i):
        lim = math.sqrt(6.0 / (i + o))
        return rng.uniform(-lim, lim, size=(o, i)).astype(np.float32)

    ws = [xavier(64, 32), xavier(16, 64), xavier(64, 32), xavier(64, 64), xavier(16, 64)]
    grid = rng.uniform(-grid_range, grid_range, size=n_params(desc) - N_MLP).astype(np.float32)
    return np.concatenate([w.ravel() for w in ws] + [grid]).astype(np.float16)


def make_coords(rng, n, margin=0.0, lt=None):
    """positions U(0.02, 0.98), dt unused, unit directions mapped to [0, 1].  margin > 0 (with lt): no position closer than `margin` cells to a cell face of any level."""
    c = rng.uniform(0.02, 0.98, size=(n, 7)).astype(np.float32)
    if margin > 0.0:
        for _ in range(200):
            bad = np.zeros(n, bool)
            for l in range(16):
                p = lt[0][l].astype(np.float64) * c[:, :3].astype(np.float64) + 0.5
                f = p - np.floor(p)
                bad |= ((f < margin) | (f > 1.0 - margin)).any(axis=1)
            if not bad.any():
                break
            c[bad, :3] = rng.uniform(0.02, 0.98, size=(int(bad.sum()), 3)).astype(np.float32)
        assert not bad.any()
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    c[:, 4:7] = (d + 1) / 2
    return c


class _RoundGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.float16).to(torch.float64)


def round_fp16(x):
    """an fp16 rounding point of the forward pass, straight-through"""
    return x + (x.detach().to(torch.float16).to(torch.float64) - x.detach())


def identity(x):
    return x


def sh4(d01):
    x, y, z = (d01[:, i] * 2 - 1 for i in range(3))
    xy, xz, yz, x2, y2, z2 = x * y, x * z, y * z, x * x, y * y, z * z
    o = [0.28209479177387814 + 0 * x, -0.48860251190291987 * y, 0.48860251190291987 * z, -0.48860251190291987 * x, 1.0925484305920792 * xy, -1.0925484305920792 * yz,
         0.94617469575755997 * z2 - 0.31539156525251999, -1.0925484305920792 * xz, 0.54627421529603959 * x2 - 0.54627421529603959 * y2,
         0.59004358992664352 * y * (-3 * x2 + y2), 2.8906114426405538 * xy * z, 0.45704579946446572 * y * (1 - 5 * z2), 0.3731763325901154 * z * (5 * z2 - 3),
         0.45704579946446572 * x * (1 - 5 * z2), 1.4453057213202769 * z * (x2 - y2), 0.59004358992664352 * x * (-x2 + 3 * y2)]
    return torch.stack(o, 1)


def forward(lt, params64, coords, round_back=False, rounding=round_fp16, pos64=None):
    """params64: float64 tensor [n_params]; coords: float32 numpy [n, 7] -> [n, 16] float64 (rows 0..2 rgb raw, 3 density raw, 4..15 the padding outputs).
    rounding: round_fp16, or identity for the plain float64 network.  pos64: a float64 tensor [n, 3] equal to coords[:, :3] that requires grad -- the trilinear weights
    then depend on it differentiably (the cells stay those of the float32 positions)."""
    scale, res, off, cnt, hashed = lt
    n = coords.shape[0]
    W = params64
    dW1, dW2 = W[0:2048].view(64, 32), W[2048:3072].view(16, 64)
    rW1, rW2, rW3 = W[3072:5120].view(64, 32), W[5120:9216].view(64, 64), W[9216:10240].view(16, 64)
    grid = W[N_MLP:].view(-1, 2)
    pos = coords[:, :3].astype(np.float32)
    feats = []
    for l in range(16):
        # fmaf(scale, x, 0.5) as hashgrid_encode_one has it: the product of two float32 is exact in float64 (48 bits) and so is its sum with 0.5 for positions in
        # [0, 1] (at most 50 bits), so the one rounding to float32 is the fused operation's
        p = (np.float64(scale[l]) * pos.astype(np.float64) + 0.5).astype(np.float32)
        fl = np.floor(p)
        g = fl.astype(np.int64).astype(np.uint32)
        w = (p - fl).astype(np.float32)
        if pos64 is not None:
            # the float32 weights' values (at the fine levels they differ from the exact ones by up to 1e-4: enough to flip fp16 roundings downstream), the exact derivative
            w_t = float(scale[l]) * pos64
            w_t = torch.from_numpy(w.astype(np.float64)) + (w_t - w_t.detach())
        acc = 0
        for c in range(8):
            wt = np.ones(n, np.float32)
            wt_t = 1.0
            gl = []
            for d in range(3):
                if (c >> d) & 1:
                    wt = wt * w[:, d]
                    gl.append(g[:, d] + np.uint32(1))
                    if pos64 is not None:
                        wt_t = wt_t * w_t[:, d]
                else:
                    wt = wt * (np.float32(1) - w[:, d])
                    gl.append(g[:, d])
                    if pos64 is not None:
                        wt_t = wt_t * (1.0 - w_t[:, d])
            if hashed[l]:
                idx = gl[0] ^ (gl[1] * np.uint32(2654435761)) ^ (gl[2] * np.uint32(805459861))
            else:
                idx = gl[0] + gl[1] * res[l] + gl[2] * res[l] * res[l]
            e = (idx % cnt[l]).astype(np.int64) + int(off[l])
            weight = wt_t if pos64 is not None else torch.from_numpy(wt.astype(np.float64))
            acc = acc + weight[:, None] * grid[torch.from_numpy(e)]
        feats.append(acc)
    rg = _RoundGrad.apply if round_back else identity
    x = rg(rounding(torch.cat(feats, 1)))
    h = rg(rounding(torch.relu(x @ dW1.T)))
    dout = rg(rounding(h @ dW2.T))
    sh = rounding(sh4(torch.from_numpy(coords[:, 4:7].astype(np.float64))))
    rin = torch.cat([dout, sh], 1)
    h1 = rg(rounding(torch.relu(rin @ rW1.T)))
    h2 = rg(rounding(torch.relu(h1 @ rW2.T)))
    o = rounding(h2 @ rW3.T)
    return torch.cat([o[:, :3], dout[:, :1], o[:, 4:].detach()], 1)


def gradient(lt, p16, coords, dl, round_back=False, want_input=False):
    """dL/dparams (float64 numpy) of L = sum(out * dl) at the fp16 blob p16; dl: float [n, 16] (rows 4..15 ignored).  round_back: dl is scaled by LOSS_SCALE and cast
    to fp16 first and the result divided by the scale, as a caller of the kernel does.  want_input: also dL/dposition [n, 3] (weights differentiable)."""
    P = torch.from_numpy(np.asarray(p16).astype(np.float64)).requires_grad_(True)
    pos64 = torch.from_numpy(coords[:, :3].astype(np.float64)).requires_grad_(True) if want_input else None
    out = forward(lt, P, coords, round_back=round_back, pos64=pos64)
    DL = torch.from_numpy(np.nan_to_num(np.asarray(dl, np.float64)))
    DL[:, 4:] = 0
    s = 1.0
    if round_back:
        s = LOSS_SCALE
        DL = (DL * s).to(torch.float16).to(torch.float64)
    wanted = [P] + ([pos64] if want_input else [])
    gs = torch.autograd.grad((out * DL).sum(), wanted)
    res = [(g / s).numpy() for g in gs]
    return res if want_input else res[0]


def block_errors(lt, got, want):
    """relative L2 error per block: ||got - want|| / ||want|| (blocks whose expected gradient is zero must be zero: error 0 or inf)"""
    out = {}
    for name, a, b in blocks(lt):
        nw = np.linalg.norm(want[a:b])
        ne = np.linalg.norm(np.asarray(got[a:b], np.float64) - want[a:b])
        out[name] = (ne / nw) if nw > 0 else (0.0 if ne == 0 else float("inf"))
    return out


def fit_loop(lt, teacher16, student16, coords, steps=20, lr=1e-2, round_back=False):
    """The end-to-end loop on the CPU: fp32 master, fp16 parameters in the forward, mean square over channels 0..3, Adam(lr, eps=1e-15).  -> losses[steps + 1]"""
    target = forward(lt, torch.from_numpy(teacher16.astype(np.float64)), coords).detach()[:, :4]
    master = torch.from_numpy(student16.astype(np.float32)).requires_grad_(True)
    opt = torch.optim.Adam([master], lr=lr, eps=1e-15)
    losses = []
    for step in range(steps + 1):
        p = master.detach().to(torch.float16).to(torch.float64).requires_grad_(True)
        loss = ((forward(lt, p, coords, round_back=round_back)[:, :4] - target) ** 2).mean()
        losses.append(loss.item())
        if step == steps:
            break
        s = LOSS_SCALE if round_back else 1.0
        gp, = torch.autograd.grad(loss * s, p)
        master.grad = (gp / s).to(torch.float32)
        opt.step()
    return losses, target
