"""CPU twin of the trainable environment map (include/nrs.h, "the environment map"), written from the text there, not from the kernels.

numpy float32 in the written order wherever the header fixes an order, Python integers for the cells:

    footprint64            the lookup's continuous texel coordinates, angles in float64 (what the device's acosf / atan2f approximate)
    split_footprint        (tx, ty, wx, wy) of continuous coordinates, as the device splits them
    lookup                 the bilinear read at a footprint: wrap in x, clamp in y, ((w00 a + w10 b) + w01 c) + w11 e in float32
    background_linear      env.rgb + srgb_to_linear(bg) * (1 - env.a)
    aux_record             the per-slot record of nrs_ray_loss_ex on top of ray_loss_ref's composite, in float64 or float32
    quantise / deposit     the deposit rule; accumulate_cells: the cells of one accumulate call as exact integers
    cells_to_gradient      (float)((double)cell * 2^-32)
    step                   the envmap's step through optimizer_ref (n_matrix = 0)
"""
import math

import numpy as np
import torch

import optimizer_ref
import ray_loss_ref as rl

F = np.float32
CLAMP = 512.0
SCALE = 4294967296.0  # 2^32
ENVMAP_HYPER = optimizer_ref.Hyper(beta1=0.9, beta2=0.99, epsilon=1e-10, l2_reg=0.0, non_matrix_lr_factor=1.0, ema_decay=0.99)


# ---- the lookup ---------------------------------------------------------------------------------------------------------------------------------------------------
def footprint64(dirs, res_x, res_y):
    """continuous texel coordinates (fx, fy) of float32 directions [n, 3], everything in float64: theta = acos(clamp(d.y)), phi = atan2(-d.x, d.z)"""
    d = np.asarray(dirs, F).astype(np.float64)
    theta = np.arccos(np.clip(d[:, 1], -1.0, 1.0))
    phi = np.arctan2(-d[:, 0], d[:, 2])
    return (phi / (2.0 * math.pi) + 0.5) * (res_x - 1), theta / math.pi * (res_y - 1)


def split_footprint(fx, fy):
    """truncate towards zero, the fraction is the weight: int32 tx, ty and float32 wx, wy of float32 coordinates"""
    fx, fy = np.asarray(fx, F), np.asarray(fy, F)
    tx, ty = fx.astype(np.int32), fy.astype(np.int32)
    return tx, ty, (fx - tx.astype(F)).astype(F), (fy - ty.astype(F)).astype(F)


def corners(tx, ty, res_x, res_y):
    """the four texels of a footprint, in deposit order: x wraps once and is then clamped into the map, y clamps"""
    def wrap(x):
        x = int(x)
        x = x + res_x if x < 0 else (x - res_x if x >= res_x else x)
        return min(max(x, 0), res_x - 1)

    def clamp(y):
        return min(max(int(y), 0), res_y - 1)
    x0, x1, y0, y1 = wrap(tx), wrap(int(tx) + 1), clamp(ty), clamp(int(ty) + 1)
    return (x0, y0), (x1, y0), (x0, y1), (x1, y1)


def weights(wx, wy):
    """(1 - wx) * (1 - wy), wx * (1 - wy), (1 - wx) * wy, wx * wy in float32, in that order"""
    wx, wy = F(wx), F(wy)
    one = F(1)
    with np.errstate(all="ignore"):
        return [F(F(one - wx) * F(one - wy)), F(wx * F(one - wy)), F(F(one - wx) * wy), F(wx * wy)]


def lookup(texels, tx, ty, wx, wy):
    """[n, 4] float32: the bilinear read of texels [res_y, res_x, 4] at n footprints"""
    tex = np.asarray(texels, F)
    res_y, res_x = tex.shape[:2]
    out = np.zeros((len(tx), 4), F)
    for k in range(len(tx)):
        (ax, ay), (bx, by), (cx, cy), (ex, ey) = corners(tx[k], ty[k], res_x, res_y)
        w = weights(wx[k], wy[k])
        a, b, c, e = tex[ay, ax], tex[by, bx], tex[cy, cx], tex[ey, ex]
        out[k] = ((w[0] * a + w[1] * b).astype(F) + (w[2] * c).astype(F)).astype(F) + (w[3] * e).astype(F)
    return out


def srgb_to_linear32(s):
    """the ray loss's curve in float32 with a correctly rounded pow (ray_loss_ref's convention)"""
    s = np.asarray(s, F)
    hi = np.power(((np.maximum(s, F(0.04045)) + F(0.055)).astype(F) / F(1.055)).astype(np.float64), 2.4).astype(F)
    return np.where(s <= F(0.04045), (s / F(12.92)).astype(F), hi).astype(F)


def background_linear(texels, tx, ty, wx, wy, bg_srgb):
    """[n, 3] float32: env.rgb + srgb_to_linear(bg) * (1 - env.a)"""
    env = lookup(texels, tx, ty, wx, wy)
    rest = (F(1) - env[:, 3:4]).astype(F)
    return (env[:, :3] + (srgb_to_linear32(bg_srgb) * rest).astype(F)).astype(F)


# ---- the aux record -----------------------------------------------------------------------------------------------------------------------------------------------
def aux_record(b, bg_linear, dtype=torch.float64):
    """What nrs_ray_loss_ex writes per slot when d_background_linear is given: dict of g [R, 3], T [R], target [R, 3], C [R, 3], n [R], M [R], near_threshold [R].
    The composite (M, T and the colour in front of the background) is ray_loss_ref's, run with a black background; the target and the background term are
    src/testbed_nerf.cu:1808-1828 on bg_linear."""
    out = torch.as_tensor(np.asarray(b["out"], np.float64)).to(dtype)
    black = dict(b, background=np.zeros((b["numsteps"].shape[0], 3), F))
    with torch.no_grad():
        f = rl._forward(black, dtype, out)
        p = b["p"]
        bg = torch.as_tensor(np.asarray(bg_linear, F).astype(np.float64)).to(dtype)
        tex = torch.as_tensor(np.asarray(b["target"], F).astype(np.float64)).to(dtype)
        a = tex[:, 3:4]
        if p["lin"] or p["color_space"] == rl.LINEAR:
            target = tex[:, :3] + (1.0 - a) * bg
            if not p["lin"]:
                target, bg = rl.linear_to_srgb(target), rl.linear_to_srgb(bg)
        else:
            bg = rl.linear_to_srgb(bg)
            safe = torch.where(a > 0, a, torch.ones_like(a))
            target = torch.where(a > 0, rl.linear_to_srgb(tex[:, :3] / safe) * a + (1.0 - a) * bg, bg)
        C = f.C + torch.where((f.M == f.N)[:, None], f.T[:, None] * bg, torch.zeros((), dtype=dtype))
        _, g = rl.loss_and_gradient(p["loss_type"], target, C)
    return dict(g=g.numpy(), T=f.T.numpy(), target=target.numpy(), C=C.numpy(), n=f.N.numpy(), M=f.M.numpy(), near_threshold=f.near_threshold.numpy(), live=f.live)


def split_aux(aux_words):
    """the device's [R, 12] int32 words as the record's fields"""
    w = np.ascontiguousarray(aux_words).view(np.uint32).reshape(-1, 12)
    fl = w.view(F)
    return dict(g=fl[:, 0:3], T=fl[:, 3], target=fl[:, 4:7], C=fl[:, 7:10], n=w[:, 10], M=w[:, 11])


# ---- the gradient -------------------------------------------------------------------------------------------------------------------------------------------------
def loss_gradient32(kind, target, pred):
    """loss_and_gradient's gradient of one channel in float32, in the kernel's written order (L2 and RelativeL2: what the exact tests use)"""
    target, pred = F(target), F(pred)
    diff = F(pred - target)
    if kind == rl.L2:
        return F(F(2.0) * diff)
    if kind == rl.RELATIVE_L2:
        f = F(F(1.0) / F(F(pred * pred) + F(1e-2)))
        return F(F(F(2.0) * diff) * f)
    raise ValueError(kind)


def quantise(p):
    """one deposit as an integer: 0 unless p (a float32) is finite and non-zero; clamped to +-512, times 2^32 (exact), rounded to nearest even"""
    p = float(F(p))
    if not math.isfinite(p) or p == 0.0:
        return 0
    p = min(max(p, -CLAMP), CLAMP)
    return int(round(p * SCALE))  # Python's round: ties to even; the product is exact in float64


def deposit(cells, res_x, res_y, tx, ty, wx, wy, v):
    """the twelve deposits of one slot into cells [res_y][res_x][4] (a flat list of Python integers)"""
    for (x, y), w in zip(corners(tx, ty, res_x, res_y), weights(wx, wy)):
        for c in range(3):
            with np.errstate(all="ignore"):
                cells[4 * (x + y * res_x) + c] += quantise(F(F(v[c]) * w))


def slot_value(aux, s, bg_linear, loss_type, envmap_loss_type, loss_scale, n_rays, lin):
    """v[3] of slot s in float32, in the header's order; the sRGB divisor's pow through float64 (correctly rounded)"""
    lg = [F(aux["g"][s, c]) for c in range(3)]
    if envmap_loss_type != loss_type:
        lg = [loss_gradient32(envmap_loss_type, aux["target"][s, c], aux["C"][s, c]) for c in range(3)]
    scale = F(F(loss_scale) / F(n_rays))
    v = []
    for c in range(3):
        with np.errstate(all="ignore"):
            dbg = F(F(aux["T"][s]) * lg[c])
            if not lin:
                dbg = F(dbg / srgb_to_linear_derivative32(linear_to_srgb32(bg_linear[s, c])))
            v.append(F(scale * dbg))
    return v


def linear_to_srgb32(v):
    v = F(v)
    return F(F(12.92) * v) if v < F(0.0031308) else F(F(F(1.055) * F(math.pow(float(v), float(F(0.41666))))) - F(0.055))


def srgb_to_linear_derivative32(s):
    s = F(s)
    if s <= F(0.04045):
        return F(F(1.0) / F(12.92))
    return F(F(F(2.4) / F(1.055)) * F(math.pow(float(F(F(s + F(0.055)) / F(1.055))), float(F(1.4)))))


def deposits(aux, numsteps_out, live):
    """which slots deposit: below the counter, with samples, neither stopped nor clipped"""
    n = aux["n"].astype(np.int64)
    ok = (np.arange(len(n)) < live) & (n > 0) & (np.asarray(numsteps_out)[:, 0].astype(np.int64) == n)
    return ok


def accumulate_cells(res_x, res_y, n_rays, live, numsteps_out, aux, bg_linear, footprint, loss_type, envmap_loss_type, loss_scale, lin, cells=None):
    """The cells after one nrs_envmap_accumulate on zero cells (or on `cells`): a flat list of Python integers [res_y * res_x * 4].  aux: split_aux of the device's
    words or a dict of float32 arrays; footprint [R, 4] int32 (tx, ty, bits of wx, wy)."""
    cells = [0] * (4 * res_x * res_y) if cells is None else list(cells)
    fp = np.ascontiguousarray(footprint).view(np.int32).reshape(-1, 4)
    w = fp[:, 2:4].copy().view(F)
    ok = deposits(aux, numsteps_out, live)
    for s in np.nonzero(ok)[0]:
        v = slot_value(aux, s, np.asarray(bg_linear, F), loss_type, envmap_loss_type, loss_scale, n_rays, lin)
        deposit(cells, res_x, res_y, int(fp[s, 0]), int(fp[s, 1]), w[s, 0], w[s, 1], v)
    return cells


def cells_to_gradient(cells):
    """(float)((double)cell * 2^-32) per cell"""
    return np.array([F(float(c) * 2.0 ** -32) for c in cells], F)


def fresh_state(texels):
    t = np.asarray(texels, F).reshape(-1)
    z = np.zeros_like(t)
    return optimizer_ref.State(t.copy(), z.copy(), z.copy(), np.zeros(t.size, np.uint32), t.copy(), t.astype(np.float16), 0)


def step(state, grad, loss_scale, lr, twin=optimizer_ref.twin64, fp16_for_ema=None, hyper=ENVMAP_HYPER):
    """one nrs_envmap_step on `state` with the float gradient `grad`: every texel channel is a non-matrix parameter"""
    return twin(state, np.asarray(grad, F), hyper, 0, loss_scale, lr, fp16_for_ema=fp16_for_ema)
