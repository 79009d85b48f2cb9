"""CPU twins of the training-ray path (include/nrs.h, "training rays"): the ray loss with its gradient, and the sample generator.

A batch is a dict:
    out        [n, 4] float64   raw network outputs of every sample (rgb, density), values an fp16 holds
    coords     [n, ld] float32  the samples' records (warped position, warped dt, warped direction, padding)
    numsteps   [R, 2] int64     (count, base) per ray slot
    target     [R, 4] float32   linear premultiplied rgba;  background [R, 3] float32 (sRGB) or None;  origins [R, 3] float32 or None
    p          dict: loss_type, loss_scale, color_space, lin (train_in_linear_colors), background (3), near_distance, l1 (density_l1_reg), cap (max_samples_compacted)
    rgb_act, den_act, aabb = (min[3], max[3]), live (rays below the counter; R when absent)

composite_loss   float64, dL/doutput from autograd of s * sum over rays and channels of L, plus the three additive terms the reference adds with no loss behind them
closed_form      the reference's formula (T after the sample, suffix = C - C2), float64
closed_form32    the same in float32: the reference's own arithmetic
march            the generator's walk in numpy float32 on the oracle's exported scalars
large_scene_walk that walk in a box of side 4 or 16 through block_bitfield on large_scene_rays (with and without the cone): the generator's large-box cases
big_box_batch    random_batch at a cone's steps (dt of 1..128 minimum steps) in such a box, with the near-distance term

All three loss twins run the rays side by side and the samples of a ray one after the other, so a ray's sums are formed in the reference's order.
"""
import ctypes as C

import numpy as np
import torch

EPS = 1e-4
L2, L1, MAPE, SMAPE, HUBER, LOG_L1, RELATIVE_L2 = range(7)
ACT_NONE, ACT_RELU, ACT_LOGISTIC, ACT_EXPONENTIAL = range(4)
LINEAR, SRGB = 0, 1
MIN_STEP = float(np.float32(np.float32(1.73205080757) / np.float32(1024)))
MAX_STEPSIZE = float(np.float32(np.float32(MIN_STEP) * np.float32(16)))
DT_SPAN = float(np.float32(np.float32(MAX_STEPSIZE) - np.float32(MIN_STEP)))


def _exp(x):
    """exp / log / pow of the float32 twin are the correctly rounded ones (through float64), so that closed_form32 is the same on every CPU: the vectorised float32
    kernels of torch differ by an ulp between instruction sets, which moves the twin's worst error from machine to machine"""
    return torch.exp(x.double()).float() if x.dtype == torch.float32 else torch.exp(x)


def _log(x):
    return torch.log(x.double()).float() if x.dtype == torch.float32 else torch.log(x)


def _pow(x, e):
    return torch.pow(x.double(), e).float() if x.dtype == torch.float32 else torch.pow(x, e)


def unwarp_dt(w):
    return w * DT_SPAN + MIN_STEP


def warp_dt_of(dt):
    """float32 warped value whose unwarp is close to dt (for building batches)"""
    return np.float32((np.float64(dt) - MIN_STEP) / DT_SPAN)


def rgb_act(x, act):
    if act == ACT_RELU:
        return torch.clamp(x, min=0)
    if act == ACT_LOGISTIC:
        return 1.0 / (1.0 + _exp(-x))
    if act == ACT_EXPONENTIAL:
        return _exp(torch.clamp(x, -10.0, 10.0))
    return x


def rgb_act_derivative(x, act):
    if act == ACT_RELU:
        return (x > 0).to(x.dtype)
    if act == ACT_LOGISTIC:
        s = 1.0 / (1.0 + _exp(-x))
        return s * (1 - s)
    if act == ACT_EXPONENTIAL:
        return _exp(torch.clamp(x, -10.0, 10.0))
    return torch.ones_like(x)


def den_act(x, act):
    if act == ACT_RELU:
        return torch.clamp(x, min=0)
    if act == ACT_LOGISTIC:
        return 1.0 / (1.0 + _exp(-x))
    if act == ACT_EXPONENTIAL:
        return _exp(x)
    return x


def den_act_derivative(x, act):
    if act == ACT_RELU:
        return (x > 0).to(x.dtype)
    if act == ACT_LOGISTIC:
        s = 1.0 / (1.0 + _exp(-x))
        return s * (1 - s)
    if act == ACT_EXPONENTIAL:
        return _exp(torch.clamp(x, -15.0, 15.0))
    return torch.ones_like(x)


def srgb_to_linear(s):
    return torch.where(s <= 0.04045, s / 12.92, _pow((torch.clamp(s, min=0.04045) + 0.055) / 1.055, 2.4))


def linear_to_srgb(v):
    return torch.where(v < 0.0031308, 12.92 * v, 1.055 * _pow(torch.clamp(v, min=0.0031308), 0.41666) - 0.055)


def loss_and_gradient(kind, target, pred):
    """per channel: (loss, d loss / d pred) as the reference writes them (Huber with alpha = 1).  The reference's gradient of the three normalised losses (relative
    L2, MAPE, SMAPE) holds the normaliser fixed; so does the loss here when autograd differentiates it."""
    d = pred - target
    pf = pred.detach()
    one = torch.ones_like(d)
    sign = torch.where(torch.signbit(d), -one, one)  # copysign(1, d)
    if kind == L2:
        return d * d, 2.0 * d
    if kind == RELATIVE_L2:
        f = 1.0 / (pf * pf + 1e-2)
        return d * d * f, 2.0 * d * f
    if kind == L1:
        return d.abs(), sign
    if kind == MAPE:
        f = 1.0 / (pf.abs() + 1e-2)
        return d.abs() * f, sign * f
    if kind == SMAPE:
        f = 1.0 / (0.5 * (pf.abs() + target.abs()) + 1e-2)
        return d.abs() * f, sign * f
    if kind == HUBER:
        big = d.abs() > 1.0
        return torch.where(big, d.abs() - 0.5, 0.5 * d * d), torch.where(big, torch.where(d > 0, one, -one), d)
    if kind == LOG_L1:
        div = d.abs() + 1.0
        return _log(div), sign / div
    raise ValueError(kind)


def kink_distance(kind, target, pred):
    """how far pred - target is from a point where the loss has no derivative (inf where there is none)"""
    d = (pred - target).abs()
    if kind in (L1, MAPE, SMAPE, LOG_L1):
        return d
    if kind == HUBER:
        return (d - 1.0).abs()
    return torch.full_like(d, float("inf"))


class Forward:
    pass


def _forward(b, dtype, out):
    """The first loop of the reference, the target and the loss: everything per ray."""
    f = Forward()
    ns = torch.as_tensor(np.asarray(b["numsteps"], np.int64))
    R = ns.shape[0]
    n = out.shape[0]
    live = int(b.get("live", R))
    ray = torch.arange(R)
    count, base = ns[:, 0], ns[:, 1]
    inside = (base <= n) & (count <= n - torch.clamp(base, max=n)) & (count <= 1024)
    N = torch.where((ray < live) & inside, count, torch.zeros_like(count))
    wdt = torch.as_tensor(np.asarray(b["coords"])[:, 3].astype(np.float64)).to(dtype)
    T = torch.ones(R, dtype=dtype)
    Cc = torch.zeros(R, 3, dtype=dtype)
    M = torch.zeros(R, dtype=torch.int64)
    near_threshold = torch.zeros(R, dtype=torch.bool)
    in_band = torch.zeros(R, dtype=torch.bool)  # some transmittance in front of a sample within a factor 2 of the threshold
    for j in range(int(N.max()) if R else 0):
        at = (j < N) & (M == j)  # the ray reaches the test in front of sample j
        if not bool(at.any()):
            break
        near_threshold |= at & ((T.detach() - EPS).abs() <= 1e-3 * EPS)
        in_band |= at & (T.detach() >= 0.5 * EPS) & (T.detach() <= 2.0 * EPS)
        act = at & (T.detach() >= EPS)
        idx = torch.clamp(base + j, max=max(n - 1, 0))
        o = out[idx]
        rgb = rgb_act(o[:, :3], b["rgb_act"])
        alpha = 1.0 - _exp(-den_act(o[:, 3], b["den_act"]) * unwarp_dt(wdt[idx]))
        w = alpha * T
        Cc = Cc + torch.where(act[:, None], w[:, None] * rgb, torch.zeros((), dtype=dtype))
        T = torch.where(act, T * (1.0 - alpha), T)
        M = M + act.to(torch.int64)
    p = b["p"]
    bg = b["background"]
    bg = torch.as_tensor(np.asarray(bg, np.float32).astype(np.float64)).to(dtype) if bg is not None else \
        torch.as_tensor(np.asarray(p["background"], np.float32).astype(np.float64)).to(dtype).expand(R, 3)
    bg = srgb_to_linear(bg)
    tex = torch.as_tensor(np.asarray(b["target"], np.float32).astype(np.float64)).to(dtype)
    a = tex[:, 3:4]
    if p["lin"] or p["color_space"] == LINEAR:
        target = tex[:, :3] + (1.0 - a) * bg
        if not p["lin"]:
            target, bg = linear_to_srgb(target), linear_to_srgb(bg)
    else:
        bg = linear_to_srgb(bg)
        safe = torch.where(a > 0, a, torch.ones_like(a))
        target = torch.where(a > 0, linear_to_srgb(tex[:, :3] / safe) * a + (1.0 - a) * bg, bg)
    Cc = Cc + torch.where((M == N)[:, None], T[:, None] * bg, torch.zeros((), dtype=dtype))
    # compaction in input order
    Ml = torch.where(ray < live, M, torch.zeros_like(M))
    cbase = torch.cumsum(Ml, 0) - Ml
    cap = int(p["cap"])
    Mc = torch.minimum(cap - torch.clamp(cbase, max=cap), Ml)
    L, g = loss_and_gradient(p["loss_type"], target, Cc)
    f.R, f.n, f.live, f.N, f.M, f.Mc, f.cbase, f.base, f.T, f.C, f.target, f.bg, f.L, f.g = R, n, live, N, M, Mc, cbase, base, T, Cc, target, bg, L, g
    f.counted = (Mc > 0) & (ray < live)
    f.loss = torch.where(f.counted, L.sum(1) / 3.0 / float(b["n_rays"] if "n_rays" in b else R), torch.zeros((), dtype=dtype))
    f.counter = int(Ml.sum())
    f.near_threshold, f.in_band = near_threshold, in_band
    f.wdt = wdt
    return f


def _additive_terms(b, f, out, dtype):
    """[n, 4] what the reference adds to the gradient of every replayed sample without a loss behind it, not scaled by s except the rgb regulariser"""
    p = b["p"]
    n = out.shape[0]
    s = float(p["loss_scale"]) / float(b.get("n_rays", f.R))
    add = torch.zeros(n, 4, dtype=dtype)
    if b["rgb_act"] == ACT_EXPONENTIAL:
        add[:, :3] = s * torch.clamp(1e-4 * out[:, :3], min=0)
    if p["l1"]:
        add[:, 3] += (out[:, 3] < 0).to(dtype) * -1e-4
    return add


def _near_term(b, f, out, dtype, src, ray_of):
    p = b["p"]
    if not (p["near_distance"] > 0):
        return torch.zeros(src.shape[0], dtype=dtype)
    mn = torch.as_tensor(np.asarray(b["aabb"][0], np.float32).astype(np.float64)).to(dtype)
    mx = torch.as_tensor(np.asarray(b["aabb"][1], np.float32).astype(np.float64)).to(dtype)
    pos = torch.as_tensor(np.asarray(b["coords"])[:, :3].astype(np.float64)).to(dtype)[src]
    org = torch.as_tensor(np.asarray(b["origins"], np.float32).astype(np.float64)).to(dtype)[ray_of]
    dist = torch.sqrt((((mn + pos * (mx - mn)) - org) ** 2).sum(1))
    return ((out[src, 3] > -10.0) & (dist < float(np.float32(p["near_distance"])))).to(dtype) * 1e-4


def _compact_map(f, cap):
    """for every compact index below min(counter, cap): the sample it copies and its ray; -1 behind"""
    src = torch.full((cap,), -1, dtype=torch.int64)
    ray_of = torch.full((cap,), -1, dtype=torch.int64)
    for r in range(f.R):
        m = int(f.Mc[r]) if r < f.live else 0
        if m:
            c0, b0 = int(f.cbase[r]), int(f.base[r])
            src[c0:c0 + m] = torch.arange(b0, b0 + m)
            ray_of[c0:c0 + m] = r
    return src, ray_of


class Result:
    pass


def _closed(b, dtype):
    out = torch.as_tensor(np.asarray(b["out"], np.float64)).to(dtype)
    with torch.no_grad():
        f = _forward(b, dtype, out)
        p = b["p"]
        cap = int(p["cap"])
        s = torch.tensor(float(np.float32(p["loss_scale"])), dtype=dtype) / float(b.get("n_rays", f.R))
        src, ray_of = _compact_map(f, cap)
        dl = torch.zeros(cap, 4, dtype=dtype)
        A = torch.zeros(cap, 4, dtype=dtype)
        l2reg = 1e-4 if b["rgb_act"] == ACT_EXPONENTIAL else 0.0
        T = torch.ones(f.R, dtype=dtype)
        C2 = torch.zeros(f.R, 3, dtype=dtype)
        Mc = torch.where(torch.arange(f.R) < f.live, f.Mc, torch.zeros_like(f.Mc))
        for j in range(int(Mc.max()) if f.R else 0):
            act = j < Mc
            rows = torch.nonzero(act)[:, 0]
            idx = f.base[rows] + j
            o = out[idx]
            rgb = rgb_act(o[:, :3], b["rgb_act"])
            dt = unwarp_dt(f.wdt[idx])
            alpha = 1.0 - _exp(-den_act(o[:, 3], b["den_act"]) * dt)
            w = alpha * T[rows]
            C2[rows] = C2[rows] + w[:, None] * rgb
            T[rows] = T[rows] * (1.0 - alpha)
            suffix = f.C[rows] - C2[rows]
            g = f.g[rows]
            k = f.cbase[rows] + j
            t_rgb = s * (w[:, None] * g) * rgb_act_derivative(o[:, :3], b["rgb_act"])
            t_reg = s * torch.clamp(l2reg * o[:, :3], min=0)
            dl[k, :3] = s * ((w[:, None] * g) * rgb_act_derivative(o[:, :3], b["rgb_act"]) + torch.clamp(l2reg * o[:, :3], min=0))
            A[k, :3] = t_rgb.abs() + t_reg.abs()
            dd = den_act_derivative(o[:, 3], b["den_act"])
            inner = T[rows][:, None] * rgb - suffix
            by_mlp = dd * (dt * (g * inner).sum(1))
            l1t = (o[:, 3] < 0).to(dtype) * (-1e-4 if p["l1"] else 0.0)
            near = _near_term(b, f, out, dtype, idx, rows)
            dl[k, 3] = s * by_mlp + l1t + near
            A[k, 3] = (s * dd * dt).abs() * ((g * T[rows][:, None] * rgb).abs() + (g * suffix).abs()).sum(1) + l1t.abs() + near.abs()
    r = Result()
    r.f, r.dl, r.A, r.src, r.ray_of = f, dl, A, src, ray_of
    r.numsteps_out = torch.stack([Mc, f.cbase], 1)
    r.loss, r.counter = f.loss, f.counter
    return r


def closed_form(b):
    return _closed(b, torch.float64)


def closed_form32(b):
    return _closed(b, torch.float32)


def composite_loss(b):
    """float64; dl from autograd.  Returns a Result like closed_form's (A is closed_form's: the sizes of the terms do not depend on how the derivative is taken)."""
    dtype = torch.float64
    out = torch.as_tensor(np.asarray(b["out"], np.float64)).clone().requires_grad_(True)
    f = _forward(b, dtype, out)
    p = b["p"]
    cap = int(p["cap"])
    s = float(np.float32(p["loss_scale"])) / float(b.get("n_rays", f.R))
    objective = s * (f.L.sum(1) * f.counted.to(dtype)).sum()
    grad, = torch.autograd.grad(objective, out) if objective.requires_grad else (torch.zeros_like(out),)
    with torch.no_grad():
        outd = out.detach()
        grad = grad + _additive_terms(b, f, outd, dtype)
        src, ray_of = _compact_map(f, cap)
        ok = src >= 0
        dl = torch.zeros(cap, 4, dtype=dtype)
        dl[ok] = grad[src[ok]]
        dl[ok, 3] += _near_term(b, f, outd, dtype, src[ok], ray_of[ok])
    r = Result()
    r.f, r.dl, r.src, r.ray_of = f, dl, src, ray_of
    r.A = closed_form(b).A
    Mc = torch.where(torch.arange(f.R) < f.live, f.Mc, torch.zeros_like(f.Mc))
    r.numsteps_out = torch.stack([Mc, f.cbase], 1)
    r.loss, r.counter = f.loss.detach(), f.counter
    return r


def error_units(got, exact, A):
    """max(0, |got - v| - 2^-11 |v|) / (2^-23 A) per element: the rounding of a stored (normal) fp16 is allowed for, the rest is counted in float32 steps of the terms'
    sizes.  Where no term has a size (A == 0) the value must be exact: 0 then, inf otherwise.  Below fp16's normal range (|v| < 2^-14: a gradient at the end of a
    long ray) the stored value moves in absolute steps of 2^-24, which the allowance does not cover: there the unit counts fp16's own step, for the kernel and for
    closed_form32 stored as fp16 alike."""
    got, exact, A = (np.asarray(x, np.float64) for x in (got, exact, A))
    excess = np.maximum(0.0, np.abs(got - exact) - 2.0 ** -11 * np.abs(exact))
    with np.errstate(divide="ignore", invalid="ignore"):
        e = excess / (2.0 ** -23 * A)
    return np.where(A > 0, e, np.where(excess > 0, np.inf, 0.0))


def to_fp16_values(x):
    """what the kernel's final conversion does to an exact value: round to nearest fp16, no clamp"""
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


# ---- the generator --------------------------------------------------------------------------------------------------------------------------------------------
def ray_tmin(mn, mx, o, d):
    """BoundingBox::ray_intersect's entry distance in float32 (FLT_MAX on a miss), then max(., 0)"""
    f = np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        tmin, tmax = (mn[0] - o[0]) / d[0], (mx[0] - o[0]) / d[0]
        if tmin > tmax:
            tmin, tmax = tmax, tmin
        tymin, tymax = (mn[1] - o[1]) / d[1], (mx[1] - o[1]) / d[1]
        if tymin > tymax:
            tymin, tymax = tymax, tymin
        if tmin > tymax or tymin > tmax:
            return f(3.402823466e+38)
        if tymin > tmin:
            tmin = tymin
        if tymax < tmax:
            tmax = tymax
        tzmin, tzmax = (mn[2] - o[2]) / d[2], (mx[2] - o[2]) / d[2]
        if tzmin > tzmax:
            tzmin, tzmax = tzmax, tzmin
        if tmin > tzmax or tzmin > tmax:
            return f(3.402823466e+38)
        if tzmin > tmin:
            tmin = tzmin
    return max(f(tmin), f(0))


def march(orc_lib, bitfield, aabb, rays, jitter, cone, tmin_nudge_ulps=0, max_steps=1024, mips_out=None):
    """The generator's walk per ray, float32: returns a list of [count, 7] float32 records (warped position, warped dt, warped direction).
    tmin_nudge_ulps moves the entry distance by that many float32 steps (how stable a ray's count is against the last bit of its start).
    mips_out: a list that receives, per ray, the cascade of every sample (int array [count])."""
    f = np.float32
    bits = np.ascontiguousarray(bitfield, np.uint8)
    mn, mx = np.asarray(aabb[0], f), np.asarray(aabb[1], f)
    cone = f(cone)
    grid_vol = 128 ** 3
    records = []
    for i in range(rays.shape[0]):
        o, d = np.asarray(rays[i, :3], f), np.asarray(rays[i, 3:], f)
        tmin = ray_tmin(mn, mx, o, d)
        for _ in range(abs(int(tmin_nudge_ulps))):
            tmin = np.nextafter(tmin, f(np.inf) if tmin_nudge_ulps > 0 else f(-np.inf))
        tmin = max(tmin, f(0))
        jit = f(jitter[i]) if jitter is not None else f(0)
        t = f(tmin + f(f(orc_lib.orc_calc_dt(C.c_float(tmin), C.c_float(cone))) * jit))
        wdir = (d + f(1)) * f(0.5)
        rec, mips = [], []
        guard = 0
        while len(rec) < max_steps and guard < 200000:
            guard += 1
            pos = (o + d * t).astype(f)
            if not (np.all(pos >= mn) and np.all(pos <= mx)):
                break
            dt = f(orc_lib.orc_calc_dt(C.c_float(t), C.c_float(cone)))
            pp = pos.ctypes.data
            mip = orc_lib.orc_mip_from_dt(C.c_float(dt), pp)
            cell = orc_lib.orc_cascaded_grid_idx_at(pp, mip)
            if bits[cell // 8 + (grid_vol * mip) // 8] & (1 << (cell % 8)):
                wpos = (pos - mn) / (mx - mn)
                rec.append(np.concatenate([wpos.astype(f), [f(orc_lib.orc_warp_dt(C.c_float(dt)))], wdir.astype(f)]).astype(f))
                mips.append(mip)
                t = f(t + dt)
            else:
                t = f(orc_lib.orc_advance_to_next_voxel(C.c_float(t), C.c_float(cone), pp, d.ctypes.data, 128 >> mip))
        records.append(np.asarray(rec, f).reshape(-1, 7))
        if mips_out is not None:
            mips_out.append(np.asarray(mips, np.int64))
    return records


def layout_from_counts(counts, max_samples):
    """the deterministic order: base = exclusive sum of all counts; a ray is emitted iff it has samples and base + count <= max_samples.
    Returns (numsteps [E, 2], ray_indices [E], counters (emitted, total), bases [n])"""
    counts = np.asarray(counts, np.int64)
    bases = np.cumsum(counts) - counts
    emit = (counts > 0) & (bases + counts <= max_samples)
    idx = np.nonzero(emit)[0]
    return np.stack([counts[idx], bases[idx]], 1), idx, (int(emit.sum()), int(counts.sum())), bases


# ---- the generator in large boxes -----------------------------------------------------------------------------------------------------------------------------
GRID_VOLUME, GRID_CASCADES = 128 ** 3, 5
LARGE_SCENE_CASES = [(4, 0.0), (4, 1.0 / 256.0), (16, 0.0), (16, 1.0 / 256.0)]  # (aabb_scale, cone_angle_constant)


def scene_aabb(scale):
    """the box of side `scale` around 0.5 (float32-exact for every power of two)"""
    return ((0.5 - 0.5 * scale,) * 3, (0.5 + 0.5 * scale,) * 3)


def block_bitfield(seed, share=0.3):
    """An occupancy in which, in each of the five cascades, every block of 4 x 4 x 4 cells (64 consecutive cells in Morton order: 8 bytes) is occupied with
    probability `share`: empty space and occupied space alternate in every cascade, so both branches of the walk run everywhere."""
    blocks = np.random.default_rng(seed).random(GRID_CASCADES * GRID_VOLUME // 64) < share
    return np.repeat(np.where(blocks, 255, 0).astype(np.uint8), 8)


def large_scene_rays(scale, seed):
    """52 float32 unit rays and a jitter each for a box of side `scale`: 16 from a sphere outside the box, 16 from inside the box (0.5 +- 0.45 scale: mostly outside
    the unit cube, entry distance 0), 16 from inside the unit cube, all aimed at a point within 0.5 +- 0.3 min(scale / 2, 3); then (1, 0, 0) from outside and
    (0, -1, 0) from inside (infinite components of 1 / d), a ray that misses the box, and one that starts exactly on the face x = 0.5 - scale / 2.
    Returns (rays [52, 6], jitter [52], index of the missing ray)."""
    rng = np.random.default_rng(seed)
    f = np.float32
    o = rng.normal(size=(16, 3))
    o = 0.5 + 1.2 * np.sqrt(3.0) * scale / 2 * o / np.linalg.norm(o, axis=1, keepdims=True)
    o = np.concatenate([o, rng.uniform(0.5 - 0.45 * scale, 0.5 + 0.45 * scale, (16, 3)), rng.uniform(0.0, 1.0, (16, 3))]).astype(f)
    reach = 0.3 * min(scale / 2, 3)
    d = rng.uniform(0.5 - reach, 0.5 + reach, (48, 3)).astype(f) - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f)
    lo = 0.5 - scale / 2
    edge = np.array([[lo - 1.0, 0.5 + 0.21 * scale, 0.5 - 0.13 * scale, 1.0, 0.0, 0.0],
                     [0.5 - 0.17 * scale, 0.5 + 0.4 * scale, 0.5 + 0.11 * scale, 0.0, -1.0, 0.0],
                     [lo - 1.0, 0.5 + 0.45 * scale, 0.5, 0.6, 0.8, 0.0],   # (leaves the box's y range before it reaches its x range)
                     [lo, 0.5 + 0.1 * scale, 0.5 - 0.3 * scale, 0.6, 0.0, 0.8]], f)
    rays = np.concatenate([np.concatenate([o, d], 1), edge]).astype(f)
    return rays, rng.random(len(rays)).astype(f), 50


class LargeSceneWalk:
    pass


def large_scene_walk(orc_lib, scale, cone, seed=None):
    """The twin's walk of large_scene_rays through block_bitfield in the box of side `scale`, at the three entry distances: rays, jitter, bitfield, the records and
    cascades of the walk as it stands, its counts, which rays are stable, which start at distance 0, and the samples per cascade."""
    w = LargeSceneWalk()
    seed = 500 + scale if seed is None else seed
    w.scale, w.cone, w.aabb = scale, cone, scene_aabb(scale)
    w.rays, w.jitter, w.missing = large_scene_rays(scale, seed)
    w.bitfield = block_bitfield(seed + 1)
    w.mips = []
    with np.errstate(over="ignore", invalid="ignore"):  # (the missing ray: FLT_MAX moved up two steps, and a position at infinity)
        walks = {k: march(orc_lib, w.bitfield, w.aabb, w.rays, w.jitter, cone, tmin_nudge_ulps=k, mips_out=w.mips if k == 0 else None) for k in (-2, 0, 2)}
    counts = {k: np.array([len(r) for r in v]) for k, v in walks.items()}
    w.walk, w.counts = walks[0], counts[0]
    w.stable = (counts[-2] == counts[0]) & (counts[0] == counts[2])
    mn, mx = np.asarray(w.aabb[0], np.float32), np.asarray(w.aabb[1], np.float32)
    w.tmin = np.array([ray_tmin(mn, mx, r[:3], r[3:]) for r in w.rays])
    w.per_cascade = np.bincount(np.concatenate(w.mips), minlength=GRID_CASCADES)
    w.max_warped_dt = max((float(r[:, 3].max()) for r in w.walk if len(r)), default=0.0)
    return w


def assert_large_scene_coverage(walks):
    """What the four cases must exercise, from the twin alone: {(scale, cone): LargeSceneWalk}.  Conditions on the inputs."""
    for (scale, cone), w in walks.items():
        assert w.stable.mean() >= 0.98, (scale, cone, float(w.stable.mean()))
        assert w.counts[w.missing] == 0 and w.tmin[w.missing] > 1e38, "the missing ray misses"
        assert int((w.tmin == 0).sum()) >= 10, "cameras inside the box: entry distance 0"
        assert (w.counts > 0).sum() >= 30
    for scale, top in ((16, 4), (4, 3)):
        w = walks[scale, 1.0 / 256.0]
        assert (w.per_cascade[:top + 1] > 0).all(), (scale, w.per_cascade)
    assert walks[16, 1.0 / 256.0].max_warped_dt > 1.0, "steps beyond 16 minimum steps: a warped dt above 1"
    assert int((walks[16, 0.0].counts == 1024).sum()) >= 1, "a ray that ends on the 1024-sample limit"


# ---- batches ------------------------------------------------------------------------------------------------------------------------------------------------------
AABB_UNIT = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
CONSTRUCTED_COUNTS = [0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1024] + [1] * 64 + [3, 0, 61, 64, 1, 63]


def _half(x):
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def _layout(rng, counts, gaps):
    """bases in a shuffled order, with gaps of 0..3 records when asked: (numsteps [R, 2], n)"""
    counts = np.asarray(counts, np.int64)
    order = rng.permutation(len(counts)) if gaps else np.arange(len(counts))
    base = np.zeros(len(counts), np.int64)
    at = 0
    for r in order:
        at += int(rng.integers(0, 4)) if gaps else 0
        base[r] = at
        at += int(counts[r])
    return np.stack([counts, base], 1), at + (2 if gaps else 0)


def _params(cap, loss_type=L2, color_space=LINEAR, lin=False, loss_scale=128.0, background=(0.2, 0.5, 0.8), near_distance=0.0, l1=False):
    return dict(loss_type=loss_type, color_space=color_space, lin=bool(lin), loss_scale=float(loss_scale), background=tuple(background), near_distance=float(near_distance),
                l1=bool(l1), cap=int(cap))


def _common(rng, numsteps, n, ld, per_ray_bg, with_origins):
    R = numsteps.shape[0]
    coords = rng.random((n, ld)).astype(np.float32)
    a = rng.choice(np.array([0.0, 0.5, 1.0], np.float32), R)
    target = np.concatenate([rng.random((R, 3)).astype(np.float32) * a[:, None], a[:, None]], 1).astype(np.float32)
    bg = rng.random((R, 3)).astype(np.float32) if per_ray_bg else None
    origins = rng.random((R, 3)).astype(np.float32) if with_origins else None
    return coords, target, bg, origins


def random_batch(seed, n_rays=200, max_count=130, ld=7, gaps=True, per_ray_bg=True, rgb_act_kind=ACT_LOGISTIC, den_act_kind=ACT_EXPONENTIAL, cap=None,
                 density_mean=3.0, density_max=9.0, with_origins=False, dt_steps=(1.0, 4.0), aabb=AABB_UNIT, **params):
    """rays of 0..max_count samples; densities spread so that some rays stop early (exponential activation) and most do not.
    dt_steps: the range of a sample's dt in minimum steps -- uniform up to 4, log-uniform when the upper bound exceeds 4 (a cone's steps: up to 128), and then every
    raw density is lowered by ln(dt / MIN_STEP) before it is rounded to fp16, so that the optical depth of a sample (exponential activation) keeps the spread it has
    at short steps.  aabb: the box the batch names; origins are drawn uniform inside it (positions are warped: uniform in every box).
    The defaults give the batches this function always gave, bit for bit (tests/test_ray_loss_host.py pins one)."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, max_count + 1, n_rays)
    numsteps, n = _layout(rng, counts, gaps)
    coords, target, bg, origins = _common(rng, numsteps, n, ld, per_ray_bg, with_origins)
    wide = dt_steps[1] > 4.0
    steps = np.exp(rng.uniform(np.log(dt_steps[0]), np.log(dt_steps[1]), n)) if wide else rng.uniform(dt_steps[0], dt_steps[1], n)
    coords[:, 3] = [warp_dt_of(MIN_STEP * s) for s in steps]
    if origins is not None and aabb is not AABB_UNIT:
        mn, mx = np.asarray(aabb[0], np.float32), np.asarray(aabb[1], np.float32)
        origins = (mn + origins * (mx - mn)).astype(np.float32)
    out = np.zeros((n, 4))
    out[:, :3] = _half(rng.normal(0.0, 1.5, (n, 3)))
    ray_mean = np.zeros(n)
    for r in range(n_rays):
        ray_mean[numsteps[r, 1]:numsteps[r, 1] + numsteps[r, 0]] = rng.normal(density_mean, 1.5)
    raw = np.clip(ray_mean + rng.normal(0.0, 1.0, n), -9.0, density_max)
    if wide:
        raw = raw - np.log(unwarp_dt(coords[:, 3].astype(np.float64)) / MIN_STEP)
    out[:, 3] = _half(raw)
    total = int(counts.sum())
    return dict(out=out, coords=coords, numsteps=numsteps, target=target, background=bg, origins=origins, rgb_act=rgb_act_kind, den_act=den_act_kind, aabb=aabb,
                p=_params(total + 7 if cap is None else cap, **params))


def big_box_batch(scale, seed=None, **kw):
    """random_batch at a cone's steps in a box of side `scale`: dt of 1..128 minimum steps, Huber loss, the density regulariser, and the near-distance term at 3 / 8 of
    the box's side (6.0 at scale 16, 1.5 at scale 4) from per-ray origins inside the box."""
    return random_batch(310 + scale if seed is None else seed, dt_steps=(1.0, 128.0), aabb=scene_aabb(scale), loss_type=HUBER, l1=True, near_distance=0.375 * scale,
                        with_origins=True, **kw)


def constructed_batch(seed, ld=7, cap_slack=9, repeats=6, dt_steps=4.0, **params):
    """CONSTRUCTED_COUNTS (`repeats` times over, each time with other stops) with decisive stops: a ray either keeps its optical depth at 4.5 or below, or has one sample with sigma dt > 30 -- at sample 0, mid-chunk, either
    side of lane 31|32, the last lane of a chunk, the first of the next, the last sample but one (M == N - 1) or the last (M == N, the background term).
    Logistic colours, exponential density; every sample's dt is dt_steps minimum steps, and the densities derive from it (a stop has sigma dt > 30 from 4 steps on).
    Returns (batch, expected M per ray)."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(CONSTRUCTED_COUNTS * repeats, np.int64)
    numsteps, n = _layout(rng, counts, True)
    coords, target, bg, origins = _common(rng, numsteps, n, ld, True, False)
    coords[:, 3] = warp_dt_of(MIN_STEP * dt_steps)
    dt = float(unwarp_dt(np.float64(coords[0, 3])))
    out = np.zeros((n, 4))
    out[:, :3] = _half(rng.normal(0.0, 1.5, (n, 3)))
    expect = np.zeros(len(counts), np.int64)
    kinds = 0
    for r, (N, base) in enumerate(numsteps):
        N, base = int(N), int(base)
        if N == 0:
            continue
        depth = rng.uniform(0.5, 4.5)
        out[base:base + N, 3] = _half(np.log(depth / N / dt * rng.uniform(0.5, 1.0, N)))
        where = [None, 0, N // 2, 31, 32, 63, 64, N - 2, N - 1][kinds % 9]
        if N >= 64 or N == 1:
            kinds += 1
        else:
            where = [None, 0, N - 2, N - 1, N // 2][r % 5]
        if N == 1:
            where = [None, 0][r % 2]
        expect[r] = N
        if where is not None and 0 <= where < N:
            out[base + where, 3] = 8.5
            expect[r] = min(where + 1, N)
    total = int(expect.sum())
    b = dict(out=out, coords=coords, numsteps=numsteps, target=target, background=bg, origins=origins, rgb_act=ACT_LOGISTIC, den_act=ACT_EXPONENTIAL, aabb=AABB_UNIT,
             p=_params(total + cap_slack, **params))
    return b, expect
