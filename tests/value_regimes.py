"""Parameter blobs in the value regimes of a trained tiny-cuda-nn snapshot, and a float64 reference of the network chain that does not depend on magnitude.

Used by tests/test_gpu_value_regimes.py (on an MI355X) and tests/test_value_regimes_host.py (the same reference against the oracle's activations, no GPU).

Regimes.  Each starts from a synth.make_params blob and keeps its constant opacity channel (level 0 / feature 0 = 1, dw1[0, 0] = 1, dw2[0, 0] = sigma_raw):
  tcnn_init  table U(-1e-4, 1e-4): tiny-cuda-nn's initialisation, where the entries training never touches stay.  fp16 normals end at 6.1e-5: most of it is subnormal.
  subnormal  the same table, and column 0 of dw1 and dw2 (which multiply the constant 1.0: a bias of every unit) zero but for the constant channel's: half
             of the hidden units and nearly all density outputs are subnormal as well -- matrix products whose inputs AND results are subnormal.
  amplified  the same table, dw1 rows 1..63 times 4096 (but for column 0, the constant feature's): the subnormal features decide O(1) hidden values, densities and colours.
  wide       entries sign * 2^U(-24, 3) with exact values planted at level-0 / level-1 vertices (PLANTED), sample positions on and next to them (wide_positions).
  large      dw1 rows 1..63 times 8192 on the default table, rgbW1 times 512 (dw2 and rgbW3 scaled back): hidden activations of 10^3..10^4.
  overflow   `large` with three dw1 rows times 24 more: those hidden units leave fp16 (> 65520 -> +inf).
  zero       an all-zero table and all-zero weights but for the constants.

The interval bar (layer_interval).  One layer is got = relu?(fp16(fp32 sum of K exact fp16 x fp16 products)).  With s the exact sum (float64: exact to 2^-53) and
A = sum |x_k w_k|, a K-term fp32 sum in ANY order whose K - 1 additions each round to nearest (relative error <= 2^-24) or chop (<= 2^-23) is within
B = 2 (K - 1) 2^-24 A of s (every partial sum is bounded by A(1 + small); the factor 2 is the chop).  Rounding to fp16 and ReLU are monotone, so
relu?(fp16(s - B)) <= got <= relu?(fp16(s + B)) holds for every correct device, whatever the magnitude: no absolute-error clause.  B is derived, not measured.
For nrs_mlp_acc FP16 (the running sum rounded to fp16 after every 16-wide k step) the bound grows by one fp16 rounding (2^-11 relative, of a running sum bounded by
A) per block and one for the output: B16 = (K / 16 + 1) 2^-11 A + B."""
import numpy as np

N_DW1, N_DW2, N_RW1, N_RW2, N_RW3 = 64 * 32, 16 * 64, 64 * 32, 64 * 64, 16 * 64
N_NET = N_DW1 + N_DW2 + N_RW1 + N_RW2 + N_RW3
REGIMES = ("tcnn_init", "subnormal", "amplified", "wide", "large", "overflow", "zero")
LAYER_WIDTHS = (32, 64, 32, 64, 64)  # forward_activations of base.json: features | density hidden | density out + SH | rgb hidden 1 | rgb hidden 2
F16_MIN_NORMAL = 2.0 ** -14
# exact values planted in `wide` (fp16 bit patterns): +0, -0, +-2^-24 (smallest subnormal), 2^-14 (smallest normal), 2^-14 - 2^-24 (largest subnormal), 65504 (largest finite)
PLANTED = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x0400, 0x03ff, 0x7bff], np.uint16)


def weights(params_u16):
    """Views of the five matrices (fp16, row-major [n_out, n_in]) and the table of a base.json blob: writing through them edits the blob."""
    p = params_u16.view(np.float16)
    o = np.cumsum([0, N_DW1, N_DW2, N_RW1, N_RW2, N_RW3])
    return {"dw1": p[o[0]:o[1]].reshape(64, 32), "dw2": p[o[1]:o[2]].reshape(16, 64), "rw1": p[o[2]:o[3]].reshape(64, 32),
            "rw2": p[o[3]:o[4]].reshape(64, 64), "rw3": p[o[4]:o[5]].reshape(16, 64), "table": p[N_NET:]}


def is_subnormal(x):
    a = np.abs(np.asarray(x, np.float64))
    return (a > 0) & (a < F16_MIN_NORMAL)


def flush_subnormals(params_u16, table_only=True):
    """The mutant: the same blob with the fp16 subnormals (of the table, or of everything) replaced by zeros of their sign."""
    out = params_u16.copy()
    part = out[N_NET:] if table_only else out
    part[(part & 0x7c00) == 0] &= 0x8000
    return out


def _dense_vertex_entry(lt, level, ix, iy, iz):
    res = int(lt["resolution"][level])
    assert not lt["hashed"][level] and max(ix, iy, iz) < res
    return int(lt["offset"][level]) + ix + iy * res + iz * res * res


def wide_vertices(lt):
    """(level, ix, iy, iz, feature, fp16 bits) of the planted entries: a run along x at two (y, z) rows of level 0 (feature 1: feature 0 is the constant channel) and of level 1."""
    out = []
    for level, features in ((0, (1,)), (1, (0, 1))):
        for f in features:
            for row, (iy, iz) in enumerate(((5, 7), (6, 7))):
                for k, bits in enumerate(np.roll(PLANTED, row * 3 + f)):
                    out.append((level, 4 + k, iy, iz, f, int(bits)))
    return out


def _vertex_coordinate(scale, i):
    """The float32 x whose grid coordinate fmaf(scale, x, 0.5) (one rounding: tiny-cuda-nn's pos_fract, the kernels' cell_coords) is exactly i, for an integer i (where such a float exists): the
    sample then sits ON the vertex, with interpolation weights of exactly 1 and 0.  Between vertices (i + 0.5) the nearest float is taken."""
    x = np.float32((i - 0.5) / scale)
    if float(i) != int(i):
        return x
    cands = [x]
    for towards in (-np.inf, np.inf):
        y = x
        for _ in range(4):
            y = np.nextafter(y, np.float32(towards))
            cands.append(y)
    hits = [y for y in cands if np.float32(np.float64(scale) * np.float64(y) + 0.5) == np.float32(i)]   # (a float32 product is exact in float64)
    if hits:
        return hits[0]
    return min(cands, key=lambda y: abs(np.float64(scale) * np.float64(y) + 0.5 - i))   # no float lands on it (level 1 has such vertices): the nearest one


def wide_positions(lt):
    """[m, 3] f32 positions for `wide`: on every planted vertex, on the cell faces between neighbouring planted vertices (the middle of the edge along x, and the
    middle of the face towards the next row), and one float nextafter to either side of each of them, per axis.  A vertex i of a level sits at (i - 0.5) / scale."""
    pts = []
    for level in (0, 1):
        sc = np.float64(lt["scale"][level])
        c = lambda i, sc=sc: _vertex_coordinate(sc, i)
        for iy, iz in ((5, 7), (6, 7)):
            for k in range(len(PLANTED)):
                pts.append((c(4 + k), c(iy), c(iz)))            # on the vertex
                pts.append((c(4 + k + 0.5), c(iy), c(iz)))      # on the edge to the next one
                pts.append((c(4 + k), c(iy + 0.5), c(iz)))      # towards the other row
                pts.append((c(4 + k + 0.5), c(iy + 0.5), c(iz + 0.5)))
    p = np.asarray(pts, np.float64).astype(np.float32)
    out = [p]
    for axis in range(3):
        for towards in (-np.inf, np.inf):
            q = p.copy()
            q[:, axis] = np.nextafter(q[:, axis], np.float32(towards))
            out.append(q)
    for towards in (-np.inf, np.inf):
        out.append(np.nextafter(p, np.float32(towards)))
    return np.concatenate(out).astype(np.float32)


def make_regime(name, desc, base_params_u16, seed=2024):
    """The blob of regime `name` (uint16 bits) from a synth.make_params blob of the base.json description."""
    from nerfshop_amd import synth
    assert desc.rgb_hidden_layers == 2 and desc.density_hidden_layers == 1 and desc.sh_degree == 4
    lt = synth.level_table(desc)
    p = np.array(base_params_u16, np.uint16, copy=True)
    assert p.size == N_NET + 2 * int(lt["offset"][15] + lt["count"][15])
    w = weights(p)
    rng = np.random.Generator(np.random.PCG64(seed))
    o0, c0 = int(lt["offset"][0]), int(lt["count"][0])
    const = slice(2 * o0, 2 * (o0 + c0), 2)
    sigma_raw = w["dw2"][0, 0]
    assert (w["table"][const] == 1).all() and w["dw1"][0, 0] == 1 and not w["dw1"][0, 1:].any()

    def fill_table(values):  # in slabs: the table has 24 M entries
        t = w["table"]
        for a in range(0, t.size, 1 << 22):
            t[a:a + (1 << 22)] = values(min(1 << 22, t.size - a))
        t[const] = 1.0

    if name in ("tcnn_init", "subnormal", "amplified"):
        fill_table(lambda m: rng.uniform(-1e-4, 1e-4, size=m).astype(np.float32))
        if name == "subnormal":
            w["dw1"][1:, 0] = 0.0
            w["dw2"][1:, 0] = 0.0
        if name == "amplified":
            # a power of two: exact, max |w| ~ 1023.  Column 0 multiplies the constant feature 1.0 and stays: scaled, it is a bias of +-1000 on every hidden unit
            # that swamps the features (measured on the oracle: the frame saturates at every ray's first sample and a flushed table moves it by 2e-14)
            w["dw1"][1:, 1:] = w["dw1"][1:, 1:].astype(np.float32) * 4096.0
    elif name == "wide":
        fill_table(lambda m: (np.exp2(rng.uniform(-24.0, 3.0, size=m)) * rng.choice((-1.0, 1.0), size=m)).astype(np.float32))
        bits = w["table"].view(np.uint16)
        for level, ix, iy, iz, f, b in wide_vertices(lt):
            bits[2 * _dense_vertex_entry(lt, level, ix, iy, iz) + f] = b
    elif name in ("large", "overflow"):
        w["dw1"][1:] = w["dw1"][1:].astype(np.float32) * 8192.0           # max |w| ~ 2046
        w["dw2"][:, 1:] = w["dw2"][:, 1:].astype(np.float32) / 4096.0
        w["rw1"][:] = w["rw1"].astype(np.float32) * 512.0
        w["rw3"][:] = w["rw3"].astype(np.float32) / 512.0
        if name == "overflow":
            w["dw1"][(9, 30, 51), :] = w["dw1"][(9, 30, 51), :].astype(np.float32) * 24.0   # max |w| <= 49152: still fp16
    elif name == "zero":
        p[:] = 0
        w["table"][const] = 1.0
        w["dw1"][0, 0] = 1.0
        w["dw2"][0, 0] = sigma_raw
    else:
        raise ValueError(name)
    assert (w["table"][const] == 1).all() and w["dw1"][0, 0] == 1 and w["dw2"][0, 0] == sigma_raw and np.isfinite(p.view(np.float16)).all()
    return p


# ----------------------------------------------------------------------------------------------------------------
# the float64 reference
# ----------------------------------------------------------------------------------------------------------------
def _fp16(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def layer_interval(X, W, relu, acc16=False):
    """[lo, hi] (float64 arrays holding fp16 values, [n, n_out]) for one layer from its inputs X [n, K] (fp16 values) and weights W [n_out, K]; also s and B.
    Where s is not finite (an input is inf: the overflow regime) lo = hi = what IEEE arithmetic gives (+-inf, NaN; relu(NaN) = relu(-inf) = 0)."""
    X, W = np.asarray(X, np.float64), np.asarray(W, np.float64)
    K = X.shape[1]
    assert W.shape[1] == K and K in (32, 64)
    with np.errstate(over="ignore", invalid="ignore"):
        s = X @ W.T
        A = np.abs(X) @ np.abs(W).T
        B = 2.0 * (K - 1) * 2.0 ** -24 * A
        if acc16:
            B = (K // 16 + 1) * 2.0 ** -11 * A + B
        lo, hi = _fp16(s - B), _fp16(s + B)
        special = ~(np.isfinite(s) & np.isfinite(B))
        lo[special] = hi[special] = s[special]
        if relu:
            lo, hi = np.where(lo > 0, lo, 0.0), np.where(hi > 0, hi, 0.0)   # (NaN > 0 is False: 0, as fmax and the oracle have it)
    return lo, hi, s, B


def inside(got, lo, hi):
    got = np.asarray(got, np.float64)
    with np.errstate(invalid="ignore"):
        return ((got >= lo) & (got <= hi)) | (np.isnan(got) & np.isnan(lo))


def chain_layers(w):
    """(name, weights, relu, source of X, slice of the target it produces) of the five matrix products of the chain."""
    return (("layer1", w["dw1"], True, "layer0", "layer1"), ("layer2[:16]", w["dw2"], False, "layer1", "layer2"), ("layer3", w["rw1"], True, "layer2", "layer3"),
            ("layer4", w["rw2"], True, "layer3", "layer4"), ("outputs", w["rw3"], False, "layer4", "outputs"))


def check_chain(acts, params_u16, acc16=False):
    """acts: {"layer0": [n, 32], "layer1": [n, 64], "layer2": [n, 32], "layer3": [n, 64], "layer4": [n, 64], "outputs": [n, 16]} (fp16 values, any float dtype).
    Every layer is checked against the interval its OWN previous layer gives.  Returns {name: dict(inside share, worst |got - s| / B, share of one-value intervals)}
    and the list of failures (empty when the chain fits)."""
    w = weights(np.asarray(params_u16, np.uint16))
    report, failures = {}, []
    for name, W, relu, src, dst in chain_layers(w):
        got = np.asarray(acts[dst], np.float64)
        if dst == "layer2":
            got = got[:, :16]
        lo, hi, s, B = layer_interval(acts[src], W.astype(np.float64), relu, acc16)
        ok = inside(got, lo, hi)
        if dst == "outputs":
            # output 3 is the density output (layer 2, unit 0) copied through (nerf_network_full.h: the rgb network's output 3 is overwritten), not a row of rgbW3
            d = np.asarray(acts["layer2"], np.float64)[:, 0]
            ok[:, 3] = (got[:, 3] == d) | (np.isnan(got[:, 3]) & np.isnan(d))
        with np.errstate(invalid="ignore", divide="ignore"):
            fin = np.isfinite(s) & np.isfinite(got) & (B > 0)
            if relu:
                fin &= s > 0
            if dst == "outputs":
                fin[:, 3] = False
            ratio = np.where(fin, np.abs(got - s) / np.where(fin, B, 1.0), 0.0)
        report[name] = {"inside": float(ok.mean()), "worst_over_B": float(ratio.max()), "single_value": float((lo == hi).mean()), "n_bad": int((~ok).sum())}
        if not ok.all():
            i, j = np.argwhere(~ok)[0]
            failures.append(f"{name}: {int((~ok).sum())} of {ok.size} outside, first at sample {i} unit {j}: got {got[i, j]!r}, interval [{lo[i, j]!r}, {hi[i, j]!r}], s {s[i, j]!r}, B {B[i, j]!r}")
    return report, failures


def value_class(x):
    """0 finite, 1 +inf, 2 -inf, 3 NaN"""
    x = np.asarray(x, np.float64)
    return np.where(np.isnan(x), 3, np.where(x == np.inf, 1, np.where(x == -np.inf, 2, 0)))


def oracle_activations(model, coords7):
    """The oracle's own chain in the shape check_chain takes (256 network_activation calls + one inference: keep n small)."""
    coords7 = np.ascontiguousarray(coords7, np.float32)
    acts = {f"layer{l}": np.stack([model.network_activation(coords7, l, d) for d in range(wd)], axis=1) for l, wd in enumerate(LAYER_WIDTHS)}
    acts["outputs"] = model.inference(coords7, 1).view(np.float16).astype(np.float32)
    return acts


def coords(n, seed):
    """[n, 7] f32 network inputs: positions in the unit cube, dt, directions on the sphere mapped to [0, 1] (the suite's _rand_coords, restated so that the
    host test does not import a gpu module)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.0, 1.0, size=(n, 7)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    c[:, 4:7] = ((d + 1.0) * 0.5).astype(np.float32)
    return c


def regime_coords(name, desc, n, seed):
    """Network inputs of a regime: random ones, the cube's corners first; `wide` adds its planted positions."""
    from nerfshop_amd import synth
    c = coords(n, seed)
    c[:8, :3] = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)
    if name == "wide":
        p = wide_positions(synth.level_table(desc))
        if p.shape[0] > (n - 8) * 3 // 4:   # a small n takes an even pick of them
            p = p[np.linspace(0, p.shape[0] - 1, (n - 8) * 3 // 4).astype(np.int64)]
        c[8:8 + p.shape[0], :3] = p
    return c
