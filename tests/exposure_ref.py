"""CPU twin of per-image exposure (include/nrs.h, "per-image exposure"), written from the text there, not from the kernels.

numpy float32 operation by operation wherever the header fixes an order, Python integers for the cells:

    scale64 / targets      exp2(exposure) in float64 (what the device's expf approximates); the scaled target and the scale record at a given float32 scale
    deposits               which slots deposit
    slot_value             v[3] of one slot in float32; accumulate_cells: the cells of one accumulate call as exact integers (envmap_ref.quantise is the deposit)
    alr / pcls             the two host-side constants of a step
    step                   Adam on every image, the renormalisation and the cells' reset, in float32 (or float64: dtype=np.float64, for the error bars)
"""
import math

import numpy as np

import envmap_ref

F = np.float32
LN2 = F(0.6931471805599453)
MEAN_LANES = 1024  # the fixed order of the renormalisation's float64 sum: this many strided partial sums, then the partials in rising order


# ---- targets --------------------------------------------------------------------------------------------------------------------------------------------------------
def scale64(exposure):
    """2^exposure per image and channel in float64 from the float32 exposures"""
    return np.exp2(np.asarray(exposure, F).astype(np.float64))


def skipped(n_rays, n_images, live, ray_indices, pixels):
    """slots nrs_exposure_targets writes nothing for: at or past the counter, a ray index or an image out of range"""
    idx = np.asarray(ray_indices).astype(np.int64) & 0xffffffff
    s = np.arange(len(idx))
    ok = (s < min(live, n_rays)) & (idx < n_rays)
    img = np.full(len(idx), 1 << 40, np.int64)
    img[ok] = np.asarray(pixels).reshape(-1, 2)[idx[ok], 0].astype(np.int64) & 0xffffffff
    return ~(ok & (img < n_images))


def targets(scale, ray_indices, target_rgba):
    """d_target_out of the slots whose float32 scale [n, 3] is given: (scale * rgb, a) of the slot's ray, each product rounded once"""
    t = np.asarray(target_rgba, F)[np.asarray(ray_indices).astype(np.int64)]
    out = t.copy()
    out[:, :3] = (np.asarray(scale, F) * t[:, :3]).astype(F)
    return out


# ---- the gradient -------------------------------------------------------------------------------------------------------------------------------------------------
def deposits(n_rays, n_images, live, ray_indices, numsteps_out, scale_words):
    """which slots deposit: below the counter, a ray index in range, compact samples, and an image word in range"""
    idx = np.asarray(ray_indices).astype(np.int64) & 0xffffffff
    img = np.ascontiguousarray(scale_words).view(np.uint32).reshape(-1, 4)[:, 3].astype(np.int64)
    return (np.arange(len(idx)) < min(live, n_rays)) & (idx < n_rays) & (np.asarray(numsteps_out)[:, 0].astype(np.int64) > 0) & (img < n_images)


def slot_value(g, target, scale, pdf, loss_scale, n_rays, lin):
    """v[3] of one slot in float32, in the header's order; the sRGB divisor's pow through float64 (correctly rounded)"""
    per_ray = F(F(loss_scale) / F(n_rays))
    v = []
    for c in range(3):
        with np.errstate(all="ignore"):
            dgt = F(F(-F(g[c])) / F(pdf))
            if not lin:
                dgt = F(dgt / envmap_ref.srgb_to_linear_derivative32(target[c]))
            v.append(F(F(F(per_ray * dgt) * F(scale[c])) * LN2))
    return v


def accumulate_cells(n_rays, n_images, live, ray_indices, numsteps_out, aux, scale_words, xy_pdf, loss_scale, lin, cells=None):
    """The cells after one nrs_exposure_accumulate on zero cells (or on `cells`): a flat list of Python integers [n_images * 3].  aux: envmap_ref.split_aux of the
    device's words; scale_words [n, 4]: the device's d_scale; xy_pdf [n] by ray or None."""
    cells = [0] * (3 * n_images) if cells is None else list(cells)
    w = np.ascontiguousarray(scale_words).view(np.uint32).reshape(-1, 4)
    sc = w[:, :3].copy().view(F)
    ok = deposits(n_rays, n_images, live, ray_indices, numsteps_out, scale_words)
    for s in np.nonzero(ok)[0]:
        pdf = F(1.0) if xy_pdf is None else F(xy_pdf[int(ray_indices[s])])
        v = slot_value(aux["g"][s], aux["target"][s], sc[s], pdf, loss_scale, n_rays, lin)
        for c in range(3):
            cells[3 * int(w[s, 3]) + c] += envmap_ref.quantise(v[c])
    return cells


# ---- the step -------------------------------------------------------------------------------------------------------------------------------------------------------
def alr64(lr, beta1, beta2, t):
    """learning_rate * sqrt(1 - beta2^t) / (1 - beta1^t) in float64 from the float32 parameters"""
    lr, b1, b2 = float(F(lr)), float(F(beta1)), float(F(beta2))
    return lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)


def pcls(n_images, loss_scale, steps_between):
    return F(F(F(n_images) / F(loss_scale)) / F(steps_between))


def mean_of(values, dtype=np.float32):
    """the renormalisation's mean per channel: the float64 sum in the header's fixed order, divided by n_images and rounded once"""
    v = np.asarray(values).reshape(-1, 3)
    n = v.shape[0]
    rows = -(-n // MEAN_LANES)
    padded = np.zeros((rows * MEAN_LANES, 3), np.float64)
    padded[:n] = v.astype(np.float64)
    partial = np.zeros((MEAN_LANES, 3), np.float64)
    for r in range(rows):   # partial j adds the images j, j + MEAN_LANES, ... in rising order (an absent image adds +0.0, which changes no sum that started from +0.0)
        partial = partial + padded[r * MEAN_LANES:(r + 1) * MEAN_LANES]
    total = np.zeros(3, np.float64)
    for j in range(min(n, MEAN_LANES)):
        total = total + partial[j]
    return (total / float(n)).astype(dtype)


def step(cells, values, m, v, step_count, loss_scale, lr, beta1=0.9, beta2=0.99, epsilon=1e-8, l2_reg=0.0, steps_between=16, dtype=np.float32, alr=None):
    """one nrs_exposure_step: -> (cells (zeros), values, m, v, step_count + 1).  dtype=np.float32: every operation rounded to float32 in the header's order;
    np.float64: the same expressions on the same float32 inputs and constants without the roundings."""
    D = dtype
    cells = np.asarray(cells, np.int64).reshape(-1)
    values, m, v = (np.asarray(a, F).reshape(-1).astype(D) for a in (values, m, v))
    n_images = cells.size // 3
    t = int(step_count) + 1
    a = D(F(alr64(lr, beta1, beta2, t)) if alr is None else F(alr))
    b1, b2, eps, l2 = D(F(beta1)), D(F(beta2)), D(F(epsilon)), D(F(l2_reg))
    k = D(pcls(n_images, loss_scale, steps_between))
    one = D(1.0)
    with np.errstate(all="ignore"):
        g0 = (cells.astype(np.float64) * 2.0 ** -32).astype(F).astype(D)
        g = (g0 * k).astype(D) + (values * l2).astype(D)
        m = ((b1 * m).astype(D) + ((one - b1) * g).astype(D)).astype(D)
        v = ((b2 * v).astype(D) + ((one - b2) * (g * g).astype(D)).astype(D)).astype(D)
        values = (values - (a * (m / (np.sqrt(v).astype(D) + eps).astype(D)).astype(D)).astype(D)).astype(D)
        mean = mean_of(values, D) if D is np.float32 else values.reshape(-1, 3).mean(axis=0)
        values = (values.reshape(-1, 3) - mean).astype(D)
    return np.zeros((n_images, 3), np.int64), values.reshape(n_images, 3), m.reshape(n_images, 3), v.reshape(n_images, 3), t
