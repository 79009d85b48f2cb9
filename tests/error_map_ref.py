"""Twin of the training error map, restated from the reference's text (src/testbed_nerf.cu:983-1064 sample_cdf_2d and image_idx, :1861-1886 the deposits, :2620-2673
construct_cdf_2d / construct_cdf_1d, :3811-3822 the host loop over the images; common.h:187-210 binary_search) in numpy float32, operation for operation -- not
compiled from it.  The cells are Python ints (the library's are unsigned 64-bit fixed point: include/nrs.h, "the training error map"); the generator's draws are
dataset_ref.draws, the low-discrepancy value behind the image choice is the oracle's ld_random_val.

    quantise / cells_to_float   one deposit as the integer it adds; the float map the reference keeps, (float)cell * 2^-32
    accumulate                  the deposits of one step into a list of cells
    cdfs                        (cdf_x_cond_y, cdf_y, cdf_img, pmf_img) from a float32 map
    sample                      image, pixel, xy and pdf of every ray of nrs_dataset_rays_ex
"""
import numpy as np

import dataset_ref

f32 = np.float32
SCALE = f32(4294967296.0)
CLAMP = f32(1024.0)


# ---- the cells ----------------------------------------------------------------------------------------------------------------------------------------------------
def quantise(v):
    """float32 array -> list of Python ints: 0 unless v > 0 (NaN too), else trunc(min(v, 1024) * 2^32).  The product is exact (a power of two, no overflow) unless it
    is below 1, where it truncates to 0 whatever it rounds to."""
    v = np.asarray(v, f32).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        scaled = np.minimum(v, CLAMP) * SCALE
        keep = v > 0
    return [int(s) if k else 0 for s, k in zip(scaled.tolist(), keep.tolist())]   # (tolist: float32 -> Python float is exact, int() truncates)


def cells_to_float(cells):
    """(float)cell * 2^-32: the conversion rounds to nearest even (numpy's uint64 -> float32 cast is C's), the scaling is exact"""
    return np.array(cells, dtype=np.uint64).astype(f32) * f32(2.0 ** -32)


def accumulate(cells, shape, n_rays, counter, ray_indices, loss, xy, pixels, pdf=None):
    """Deposits into `cells` (a list of n_images * res_y * res_x Python ints, changed in place); returns loss / pdf of the live slots.  shape = (n_images, res_y, res_x)."""
    n_images, res_y, res_x = shape
    live = min(int(counter), int(n_rays))
    i = np.asarray(ray_indices).reshape(-1)[:live].astype(np.int64)
    assert (i < n_rays).all()
    xy, pixels = np.asarray(xy, f32).reshape(-1, 2), np.asarray(pixels).reshape(-1, 2)
    l = np.asarray(loss, f32).reshape(-1)[:live]
    p = np.ones(live, f32) if pdf is None else np.asarray(pdf, f32).reshape(-1)[i]
    img = pixels[i, 0].astype(np.int64)
    assert (img < n_images).all()
    rx, ry = f32(res_x), f32(res_y)
    with np.errstate(all="ignore"):
        weighted = l / p
        e = (l * f32(n_rays)) / p
        px = np.minimum(np.maximum(xy[i, 0] * rx - f32(0.5), f32(0)), rx - (f32(1.0) + f32(1e-4)))
        py = np.minimum(np.maximum(xy[i, 1] * ry - f32(0.5), f32(0)), ry - (f32(1.0) + f32(1e-4)))
        ix, iy = px.astype(np.int32), py.astype(np.int32)
        wx, wy = px - ix.astype(f32), py - iy.astype(f32)
        one = f32(1)
        products = [(one - wx) * (one - wy) * e, wx * (one - wy) * e, (one - wx) * wy * e, wx * wy * e]
    assert (ix >= 0).all() and (ix <= res_x - 2).all() and (iy >= 0).all() and (iy <= res_y - 2).all(), "the clamp of the cell index never acts"
    base = (img * res_y + iy) * res_x + ix
    for prod, off in zip(products, (0, 1, res_x, res_x + 1)):
        for at, q in zip((base + off).tolist(), quantise(prod)):
            cells[at] += q
    return weighted


# ---- the CDFs -----------------------------------------------------------------------------------------------------------------------------------------------------
MIN_PDF, MIN_PMF = f32(0.01), f32(0.1)


def _running(t):
    """the serial running sum along the last axis, every other axis in parallel"""
    out = np.empty_like(t)
    cum = np.zeros(t.shape[:-1], f32)
    for x in range(t.shape[-1]):
        cum = cum + t[..., x]
        out[..., x] = cum
    return out, cum


def _normalise(c, total, min_p):
    width = c.shape[-1]
    norm = f32(1.0) / total
    ramp = (np.arange(width, dtype=np.uint32) + 1).astype(f32)
    return (f32(1.0) - min_p) * c * norm[..., None] + min_p * ramp / f32(width)


def cdfs(data):
    """data [n_images, res_y, res_x] float32 -> (cdf_x_cond_y [n, res_y, res_x], cdf_y [n, res_y], cdf_img [n], pmf_img [n])"""
    d = np.asarray(data, f32)
    assert d.ndim == 3
    n = d.shape[0]
    c, row_total = _running(d + f32(1e-10))                        # construct_cdf_2d
    cdf_x_cond_y = _normalise(c, row_total, MIN_PDF)
    c, img_total = _running(row_total)                             # construct_cdf_1d
    cdf_y = _normalise(c, img_total, MIN_PDF)
    c, total = _running(img_total)                                 # the host loop of train_nerf
    norm = f32(1.0) / total
    pmf_img = (f32(1.0) - MIN_PMF) * img_total * norm + MIN_PMF / f32(n)
    cdf_img = _normalise(c, total, MIN_PMF)
    return cdf_x_cond_y.astype(f32), cdf_y.astype(f32), cdf_img.astype(f32), pmf_img.astype(f32)


# ---- sampling -----------------------------------------------------------------------------------------------------------------------------------------------------
def binary_search(val, rows):
    """common.h:187-210 for every ray at once: rows [n, length] is each ray's own array, val [n].  The first index whose entry is not < val, capped at length - 1."""
    n, length = rows.shape
    lanes = np.arange(n)
    first, count = np.zeros(n, np.int64), np.full(n, length, np.int64)
    while (count > 0).any():
        active = count > 0
        step = count // 2
        it = first + step
        less = active & (rows[lanes, np.minimum(it, length - 1)] < val)
        first = np.where(less, it + 1, first)
        count = np.where(less, count - (step + 1), np.where(active, step, count))
    return np.minimum(first, length - 1)


def _prev(rows, idx):
    lanes = np.arange(rows.shape[0])
    return np.where(idx > 0, rows[lanes, np.maximum(idx - 1, 0)], f32(0)).astype(f32)


def sample(seed, n_rays, n_rays_total, n_images, width, height, snap, tables, by_images, by_pixels):
    """tables = (cdf_x_cond_y [n, res_y, res_x], cdf_y [n, res_y], cdf_img [n]).  Returns {"img", "pixel" (x + y * width), "xy" [n, 2], "pdf" [n], "cdf_half" [n] bool}."""
    from oracle import ref as oref
    cdf_x_cond_y, cdf_y, cdf_img = (np.asarray(t, f32) for t in tables)
    res_y, res_x = cdf_x_cond_y.shape[1:]
    dr = dataset_ref.draws(seed, n_rays)
    i = np.arange(n_rays, dtype=np.uint32)
    lanes = np.arange(n_rays)
    with np.errstate(over="ignore"):
        img = ((((i + np.uint32(n_rays_total)) * np.uint32(n_images)) // np.uint32(n_rays)) % np.uint32(n_images)).astype(np.int64)
        img_pdf = np.ones(n_rays, f32)
        if by_images:   # image_idx, :1052-1064
            val = oref.ld_random_val(i + np.uint32(n_rays_total), np.full(n_rays, 0xdeadbeef, np.uint32), which="orc")
            rows = np.broadcast_to(cdf_img, (n_rays, n_images))
            img = binary_search(val, rows)
            img_pdf = (rows[lanes, img] - _prev(rows, img)) * f32(n_images)
    u, v = dr[:, 0].copy(), dr[:, 1].copy()
    xy_pdf = np.ones(n_rays, f32)
    half = np.zeros(n_rays, bool)
    if by_pixels:   # sample_cdf_2d, :983-1012
        half = ~(u < f32(0.5))
        uu = np.where(half, (u - f32(0.5)) / (f32(1.0) - f32(0.5)), u / f32(0.5)).astype(f32)
        rows_y = cdf_y[img]
        row = binary_search(v, rows_y)
        prev = _prev(rows_y, row)
        pmf_y = rows_y[lanes, row] - prev
        vv = (v - prev) / pmf_y
        rows_x = cdf_x_cond_y[img, row]
        col = binary_search(uu, rows_x)
        prev = _prev(rows_x, col)
        pmf_x = rows_x[lanes, col] - prev
        ux = (uu - prev) / pmf_x
        xy_pdf = np.where(half, pmf_x * pmf_y * f32(res_x * res_y), f32(1)).astype(f32)
        u = np.where(half, (col.astype(f32) + ux) / f32(res_x), uu).astype(f32)
        v = np.where(half, (row.astype(f32) + vv) / f32(res_y), v).astype(f32)
    Wf, Hf = f32(width), f32(height)
    if snap:
        u = (np.clip((u * Wf).astype(np.int32), 0, width - 1).astype(f32) + f32(0.5)) / Wf
        v = (np.clip((v * Hf).astype(np.int32), 0, height - 1).astype(f32) + f32(0.5)) / Hf
    px, py = np.clip((u * Wf).astype(np.int32), 0, width - 1), np.clip((v * Hf).astype(np.int32), 0, height - 1)
    return {"img": img.astype(np.uint32), "pixel": (px + py * width).astype(np.uint32), "xy": np.stack([u, v], 1).astype(f32), "pdf": (img_pdf * xy_pdf).astype(f32),
            "cdf_half": half}
