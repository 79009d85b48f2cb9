"""Twins of the dataset kernels, restated from the reference's text (src/testbed_nerf.cu:353-400, :1037-1186, :1777-1806; common_device.cuh:31-37, :146-243, :513-540;
src/nerf_loader.cu:164-640) in numpy -- not compiled from it.

    rays32 / rays64     generate_training_samples_nerf up to the ray, in float32 (the kernel's own expressions and order) and in float64 on the same draws
    from_rgba8_32 / 64  from_rgba32<__half>
    mark_untrained_ref  mark_untrained_density_grid in float64, with the cells whose frustum test lies within `margin` of its boundary
    read_transforms     the part of load_nerf a transforms.json folder needs, written independently of nerfshop_amd/dataset.py

A camera is its device record: 40 float32 words, [0..11] xform_start (column-major 3 x 4) | [12..23] xform_end | [24..25] focal length | [26..27] principal point |
[28..31] rolling shutter | [32] distortion mode (integer bits) | [33..39] distortion parameters.
"""
import json
import math
import os

import numpy as np

CAMERA_WORDS = 40


def camera_record(start, end=None, focal=(100.0, 100.0), pp=(0.5, 0.5), rs=(0.0, 0.0, 0.0, 0.0), mode=0, params=()):
    """start / end: 3 x 4 matrices (rows x columns)"""
    rec = np.zeros(CAMERA_WORDS, np.float32)
    start = np.asarray(start, np.float32).reshape(3, 4)
    end = start if end is None else np.asarray(end, np.float32).reshape(3, 4)
    rec[0:12], rec[12:24] = start.T.reshape(-1), end.T.reshape(-1)
    rec[24:26], rec[26:28], rec[28:32] = focal, pp, rs
    rec[32:33].view(np.uint32)[0] = mode
    rec[33:33 + len(params)] = params
    return rec


def to_struct(rec):
    """the record as an _abi.TrainingCamera"""
    from nerfshop_amd import _abi
    cam = _abi.TrainingCamera()
    cam.xform_start[:], cam.xform_end[:] = rec[0:12].tolist(), rec[12:24].tolist()
    cam.focal_length[:], cam.principal_point[:], cam.rolling_shutter[:] = rec[24:26].tolist(), rec[26:28].tolist(), rec[28:32].tolist()
    cam.distortion_mode = int(rec[32:33].view(np.uint32)[0])
    cam.distortion_params[:] = rec[33:40].tolist()
    return cam


def from_struct(cam):
    """an _abi.TrainingCamera as its 40 words (uint32: for bit comparisons)"""
    return np.frombuffer(bytes(cam), dtype=np.uint32)[1:1 + CAMERA_WORDS].copy()


# ---- the draws --------------------------------------------------------------------------------------------------------------------------------------------
_DRAWS = {}


def draws(seed, n):
    """[n, 5] float32: the five random_val draws of rays 0..n-1 (pcg32 seeded with `seed`, advanced by 8 i).  Computed once per seed with the oracle's Pcg32 and shared."""
    from oracle import oracle as orc
    have = _DRAWS.get(seed)
    if have is not None and have.shape[0] >= n:
        return have[:n]
    rng = orc.Pcg32(seed)
    base = rng.state.value
    out = np.empty((n, 5), np.float32)
    for i in range(n):
        rng.state.value = base
        rng.advance(i * 8)
        for k in range(5):
            out[i, k] = rng.next_float()
    _DRAWS[seed] = out
    return out


def rng_of(seed):
    from oracle import oracle as orc
    rng = orc.Pcg32(seed)
    return rng.state.value, rng.inc.value


# ---- lenses -------------------------------------------------------------------------------------------------------------------------------------------------
def _distort(prm, u, v):  # apply_camera_distortion, common_device.cuh:146-159
    k1, k2, p1, p2 = prm[:, 0], prm[:, 1], prm[:, 2], prm[:, 3]
    two = u.dtype.type(2)
    u2, uv, v2 = u * u, u * v, v * v
    r2 = u2 + v2
    radial = k1 * r2 + k2 * r2 * r2
    return u * radial + two * p1 * uv + p2 * (r2 + two * u2), v * radial + two * p2 * uv + p1 * (r2 + two * v2)


def _undistort(prm, u, v):  # iterative_camera_undistortion, common_device.cuh:161-200; every ray leaves the loop at its own iteration
    f = u.dtype.type
    eps, rel, max_step = f(np.float32(1.1920928955078125e-07)), f(np.float32(1e-6)), f(np.float32(1e-10))
    x00, x01 = u.copy(), v.copy()
    x0, x1 = u.copy(), v.copy()
    active = np.ones(u.shape, bool)
    for _ in range(100):
        if not active.any():
            break
        a = active
        p, y0, y1 = prm[a], x0[a], x1[a]
        step0, step1 = np.maximum(eps, np.abs(rel * y0)), np.maximum(eps, np.abs(rel * y1))
        dx0, dx1 = _distort(p, y0, y1)
        b00, b01 = _distort(p, y0 - step0, y1)
        f00, f01 = _distort(p, y0 + step0, y1)
        b10, b11 = _distort(p, y0, y1 - step1)
        f10, f11 = _distort(p, y0, y1 + step1)
        one, two = f(1), f(2)
        J00, J01 = one + (f00 - b00) / (two * step0), (f10 - b10) / (two * step1)
        J10, J11 = (f01 - b01) / (two * step0), one + (f11 - b11) / (two * step1)
        invdet = one / (J00 * J11 - J10 * J01)   # Eigen's 2 x 2 inverse: adjugate times 1 / det
        i00, i10, i01, i11 = J11 * invdet, -J10 * invdet, -J01 * invdet, J00 * invdet
        r0, r1 = y0 + dx0 - x00[a], y1 + dx1 - x01[a]
        s0, s1 = i00 * r0 + i01 * r1, i10 * r0 + i11 * r1
        x0[a], x1[a] = y0 - s0, y1 - s1
        done = s0 * s0 + s1 * s1 < max_step
        idx = np.flatnonzero(a)
        active[idx[done]] = False
    return x0, x1


def _sum3(a, b, c):  # Eigen's fixed-size reduction of three terms: a + (b + c)
    return a + (b + c)


def _rays(f, seed, cams, images, n_rays, n_rays_total, snap):
    cams = np.asarray(cams, np.float32).reshape(-1, CAMERA_WORDS)
    images = np.asarray(images)
    assert images.dtype == np.float16 and images.ndim == 4 and images.shape[3] == 4 and images.shape[0] == cams.shape[0]
    n_images, H, W = images.shape[:3]
    f32 = np.float32
    dr = draws(seed, n_rays)
    i = np.arange(n_rays, dtype=np.uint32)
    with np.errstate(over="ignore"):
        img = (((i + np.uint32(n_rays_total)) * np.uint32(n_images)) // np.uint32(n_rays)) % np.uint32(n_images)   # image_idx: 32-bit, the product wraps
    # pixel selection: single float32 operations on exact draws, the same in both twins
    u, v = dr[:, 0].copy(), dr[:, 1].copy()
    Wf, Hf = f32(W), f32(H)
    if snap:
        u = (np.clip((u * Wf).astype(np.int32), 0, W - 1).astype(f32) + f32(0.5)) / Wf
        v = (np.clip((v * Hf).astype(np.int32), 0, H - 1).astype(f32) + f32(0.5)) / Hf
    px, py = np.clip((u * Wf).astype(np.int32), 0, W - 1), np.clip((v * Hf).astype(np.int32), 0, H - 1)
    texel = images[img, py, px]
    masked = texel[:, 0].astype(f32) < 0
    target = texel.astype(f32)
    target[masked] = 0
    mb = dr[:, 2]

    # the camera of the pixel's time and the direction, in f
    C = cams[img].astype(f)
    mode = cams[img][:, 32].copy().view(np.uint32)
    uu, vv, mbb = u.astype(f), v.astype(f), mb.astype(f)
    pixel_t = C[:, 28] + C[:, 29] * uu + C[:, 30] * vv + C[:, 31] * mbb
    xf = C[:, 0:12] + (C[:, 12:24] - C[:, 0:12]) * pixel_t[:, None]
    dx = (uu - C[:, 26]) * f(W) / C[:, 24]
    dy = (vv - C[:, 27]) * f(H) / C[:, 25]
    dz = np.ones(n_rays, f)
    it = mode == 1
    if it.any():
        dx[it], dy[it] = _undistort(C[it, 33:40], dx[it], dy[it])
    ft = mode == 2
    if ft.any():  # f_theta_undistortion, common_device.cuh:231-243, error direction (0, 0, 1)
        P = C[ft, 33:40]
        xpix, ypix = (uu[ft] - C[ft, 26]) * P[:, 5], (vv[ft] - C[ft, 27]) * P[:, 6]
        norm = np.sqrt(xpix * xpix + ypix * ypix)
        alpha = P[:, 0] + norm * (P[:, 1] + norm * (P[:, 2] + norm * (P[:, 3] + norm * P[:, 4])))
        sin_a, cos_a = np.sin(alpha), np.cos(alpha)
        bad = (cos_a <= f(np.float32(1.17549435e-38))) | (norm == 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            sin_a = sin_a * (f(1) / norm)
            dx[ft], dy[ft], dz[ft] = np.where(bad, f(0), sin_a * xpix), np.where(bad, f(0), sin_a * ypix), np.where(bad, f(1), cos_a)
    d = np.stack([_sum3(xf[:, 0] * dx, xf[:, 3] * dy, xf[:, 6] * dz), _sum3(xf[:, 1] * dx, xf[:, 4] * dy, xf[:, 7] * dz),
                  _sum3(xf[:, 2] * dx, xf[:, 5] * dy, xf[:, 8] * dz)], 1)
    d = d / np.sqrt(_sum3(d[:, 0] * d[:, 0], d[:, 1] * d[:, 1], d[:, 2] * d[:, 2]))[:, None]
    d[masked] = 0
    return {"rays": np.concatenate([xf[:, 9:12], d], 1), "jitter": dr[:, 3].copy(), "target": target, "background": dr[:, 2:5].copy(),
            "pixels": np.stack([img, (px + py * W).astype(np.uint32)], 1).astype(np.uint32), "masked": masked}


def rays32(seed, cams, images, n_rays, n_rays_total=0, snap=True):
    """cams [n_images, 40] float32 records, images [n_images, H, W, 4] float16.  rays [n, 6] float32, jitter, target [n, 4], background [n, 3], pixels [n, 2] uint32."""
    return _rays(np.float32, seed, cams, images, n_rays, n_rays_total, snap)


def rays64(seed, cams, images, n_rays, n_rays_total=0, snap=True):
    """The same draws and the same pixels; the camera blend, the lens and the rotation in float64."""
    return _rays(np.float64, seed, cams, images, n_rays, n_rays_total, snap)


# ---- from_rgba32<__half> ---------------------------------------------------------------------------------------------------------------------------------
def _from_rgba8(f, pixels, white_transparent, black_transparent, mask_color, perturb_ulp=0):
    p = np.asarray(pixels, np.uint8)
    assert p.shape[-1] == 4
    inv255 = f(1.0) / f(255.0)
    rgb = p[..., :3]
    alpha = p[..., 3].astype(f) * inv255
    if white_transparent:
        alpha = np.where((rgb == 255).all(-1), f(0), alpha)
    if black_transparent:
        alpha = np.where((rgb == 0).all(-1), f(0), alpha)
    s = rgb.astype(f) * inv255
    lin = np.where(s <= f(0.04045), s / f(12.92), np.power((s + f(0.055)) / f(1.055), f(2.4)))
    if perturb_ulp:  # stand-in for a powf that is a few ulp off: every value moved by that many float32 steps, alternating in sign
        sign = np.where((np.indices(lin.shape).sum(0) & 1) == 0, 1, -1).astype(np.int32)
        moved = (lin.astype(np.float32).view(np.int32) + sign * np.int32(perturb_ulp)).view(np.float32).astype(f)
        lin = np.where(s <= f(0.04045), lin, moved)   # only what came out of the power
    out = np.concatenate([lin * alpha[..., None], alpha[..., None]], -1).astype(np.float16)
    if mask_color:
        word = p.astype(np.uint32)
        word = word[..., 0] | (word[..., 1] << 8) | (word[..., 2] << 16) | (word[..., 3] << 24)
        out[word == np.uint32(mask_color)] = np.float16(-1)
    return out


def from_rgba8_32(pixels, white_transparent=False, black_transparent=False, mask_color=0, perturb_ulp=0):
    return _from_rgba8(np.float32, pixels, white_transparent, black_transparent, mask_color, perturb_ulp)


def from_rgba8_64(pixels, white_transparent=False, black_transparent=False, mask_color=0):
    return _from_rgba8(np.float64, pixels, white_transparent, black_transparent, mask_color)


def half_steps(a, b):
    """|a - b| of two float16 arrays in units of the fp16 grid (finite values)"""
    def key(x):
        u = x.view(np.uint16).astype(np.int32)
        return np.where(u & 0x8000, -(u & 0x7fff), u)
    return np.abs(key(np.ascontiguousarray(a)) - key(np.ascontiguousarray(b)))


# ---- shared inputs of the host and GPU tests -------------------------------------------------------------------------------------------------------------
def all_pairs_image():
    """256 x 256 RGBA8 holding every (value, alpha) pair: the three colour bytes of pixel (alpha, value) are value, 255 - value, value ^ 0x55"""
    v = np.arange(256, dtype=np.uint8)
    img = np.empty((256, 256, 4), np.uint8)
    img[..., 0], img[..., 1], img[..., 2] = v[None, :], 255 - v[None, :], v[None, :] ^ 0x55
    img[..., 3] = v[:, None]
    return img


def corner_cameras(aabb_scale):
    """two cameras outside the box of this scale, looking at one of its corners"""
    cams = []
    for k, eye in enumerate(((-0.4, -0.3, -0.5), (-0.2, -0.6, -0.3))):
        lo = 0.5 - 0.5 * aabb_scale   # the box of this scale is [lo, lo + aabb_scale]^3
        eye, target = lo + aabb_scale * np.array(eye), lo + aabb_scale * np.array([0.1, 0.15, 0.05])
        z = (target - eye) / np.linalg.norm(target - eye)
        x = np.cross([0.0, 1.0, 0.2 * k], z)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        cams.append(camera_record(np.stack([x, y, z, eye], 1), focal=(70.0 + 9 * k, 64.0), pp=(0.5, 0.5)))
    return np.stack(cams)


def marked_grid(aabb_scale, seed=12):
    """A density grid for the mark_untrained tests: negative everywhere except two balls (in every cascade) that hold positive and negative cells -- one around the point
    corner_cameras look at, deep inside both frusta, one in a corner neither sees.  Positive cells that are SEEN keep their bit, and the bitfield's coarser levels
    are OR-pooled from the finer ones (as in the reference): a seen fine cell under a coarse cell whose own test fails -- the test is made at the cell's centre --
    would put a bit into an untrained cell.  Deep inside the frusta every ancestor of a seen cell is seen too, so "no bit in an untrained cell" is well defined."""
    G = 128
    noise = np.random.default_rng(seed).normal(0.02, 0.05, 5 * G ** 3).astype(np.float32)
    grid = -np.abs(noise)
    idx = np.arange(G ** 3, dtype=np.uint32)
    xyz = np.stack([_morton_invert(idx), _morton_invert(idx >> 1), _morton_invert(idx >> 2)], 1).astype(np.float64)
    lo = 0.5 - 0.5 * aabb_scale
    for level in range(5):
        pos = ((xyz + 0.5) / G - 0.5) * 2.0 ** level + 0.5
        for centre in ((0.1, 0.15, 0.05), (0.9, 0.1, 0.9)):
            ball = np.linalg.norm(pos - (lo + aabb_scale * np.array(centre)), axis=1) < 0.04 * aabb_scale + 0.02
            grid[level * G ** 3:(level + 1) * G ** 3][ball] = noise[level * G ** 3:(level + 1) * G ** 3][ball]
    return grid


# ---- mark_untrained_density_grid --------------------------------------------------------------------------------------------------------------------------
def _morton_invert(x):
    x = x & 0x49249249
    x = (x | (x >> 2)) & 0xc30c30c3
    x = (x | (x >> 4)) & 0x0f00f00f
    x = (x | (x >> 8)) & 0xff0000ff
    x = (x | (x >> 16)) & 0x0000ffff
    return x


def mark_untrained_ref(grid, cams, width, height, clear_visible, margin=1e-6):
    """(the grid afterwards, the cells whose verdict rests on a comparison within `margin` of its boundary, the cells seen) -- float64"""
    grid = np.asarray(grid, np.float32)
    cams = np.asarray(cams, np.float32).reshape(-1, CAMERA_WORDS)
    G = 128
    idx = np.arange(G ** 3, dtype=np.uint32)
    xyz = np.stack([_morton_invert(idx), _morton_invert(idx >> 1), _morton_invert(idx >> 2)], 1).astype(np.float64)
    seen_all, near_all = [], []
    for level in range(grid.size // G ** 3):
        s = 2.0 ** level
        pos = ((xyz + 0.5) / G - 0.5) * s + 0.5
        radius = 0.5 * 1.73205080757 * s / G
        seen, near = np.zeros(G ** 3, bool), np.zeros(G ** 3, bool)
        for c in cams:
            if int(c[32:33].view(np.uint32)[0]) == 2:
                seen[:] = True
                continue
            c = c.astype(np.float64)
            ploc = pos - c[9:12]
            x, y, z = ploc @ c[0:3], ploc @ c[3:6], ploc @ c[6:9]
            mx, my = z / c[24] * (width * 0.5) - (np.abs(x) - radius), z / c[25] * (height * 0.5) - (np.abs(y) - radius)
            seen |= (z > 0) & (mx > 0) & (my > 0)
            near |= (np.abs(z) < margin) | (np.abs(mx) < margin) | (np.abs(my) < margin)
        seen_all.append(seen)
        near_all.append(near)
    seen, near = np.concatenate(seen_all), np.concatenate(near_all)
    out = grid.copy()
    write = np.full(grid.shape, bool(clear_visible)) | ((grid < 0) != ~seen)
    out[write] = np.where(seen, np.float32(0), np.float32(-1))[write]
    return out, near, seen


# ---- transforms.json ------------------------------------------------------------------------------------------------------------------------------------------
def read_transforms(path):
    """{"cameras": [n, 40] float32 records, "paths": [...], "width", "height" (from w / h, or None), "aabb_scale", "scale", "offset", "white_transparent", "black_transparent"}"""
    f = np.float32
    if os.path.isdir(path):
        path = os.path.join(path, "transforms.json")
    js = json.load(open(path))
    frames = js["frames"]
    if "n_frames" in js:
        frames = frames[:int(js["n_frames"])]
    scale = f(js["scale"]) if "scale" in js else f(0.33)
    offset = np.full(3, 0.5, f)
    if "offset" in js:
        offset = np.asarray(js["offset"], f) if isinstance(js["offset"], list) else np.full(3, js["offset"], f)
    mode, prm = 0, np.zeros(7, f)
    for k, key in enumerate(["k1", "k2", "p1", "p2"]):
        if key in js:
            prm[k] = js[key]
            mode = 1 if prm[k] != 0 else mode
    pp = np.full(2, 0.5, f)
    if "cx" in js:
        pp[0] = f(js["cx"]) / f(js["w"])
    if "cy" in js:
        pp[1] = f(js["cy"]) / f(js["h"])
    rs = np.zeros(4, f)
    if "rolling_shutter" in js:
        r = js["rolling_shutter"]
        rs[:len(r[:4])] = r[:4]
    if "ftheta_p0" in js:
        prm[:] = [js["ftheta_p0"], js["ftheta_p1"], js["ftheta_p2"], js["ftheta_p3"], js["ftheta_p4"], js["w"], js["h"]]
        mode = 2

    def to_ngp(m):  # NerfDataset::nerf_matrix_to_ngp: flip y and z, scale and move the origin, cycle the axes
        m = np.asarray(m, f)[:3, :4]
        out = np.empty((3, 4), f)
        for row, src in enumerate((1, 2, 0)):
            out[row, 0], out[row, 1], out[row, 2] = m[src, 0], -m[src, 1], -m[src, 2]
            out[row, 3] = m[src, 3] * scale + offset[src]
        return out

    def focal(res, axis):
        if "fl_" + axis in js:
            return f(js["fl_" + axis])
        if "camera_angle_" + axis in js:
            deg = f(js["camera_angle_" + axis]) * f(180) / f(3.14159265358979323846)
            return f(0.5) * f(res) / f(math.tan(f(0.5) * deg * f(3.14159265358979323846) / f(180)))
        return f(0)

    width, height = js.get("w"), js.get("h")
    base = os.path.dirname(os.path.abspath(path))
    paths = []
    for fr in frames:
        p = os.path.join(base, fr["file_path"])
        paths.append(p if os.path.splitext(p)[1] else p + ".png")
    if width is None:
        from PIL import Image
        with Image.open(paths[0]) as im:
            width, height = im.size
    fx, fy = focal(int(width), "x"), focal(int(height), "y")
    if fx == 0:
        fx = fy
    if fy == 0:
        fy = fx
    cams = []
    for fr in frames:
        start = fr["transform_matrix_start"] if "transform_matrix_start" in fr else fr["transform_matrix"]
        end = fr["transform_matrix_end"] if "transform_matrix_end" in fr else start
        cams.append(camera_record(to_ngp(start), to_ngp(end), (fx, fy), pp, rs, mode, prm))
    return {"cameras": np.stack(cams), "paths": paths, "width": int(width), "height": int(height), "aabb_scale": int(js.get("aabb_scale", 1)), "scale": float(scale),
            "offset": offset, "white_transparent": bool(js.get("white_transparent", False)), "black_transparent": bool(js.get("black_transparent", False))}
