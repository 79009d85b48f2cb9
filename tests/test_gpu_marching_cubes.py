"""Mesh extraction on an MI355X: nrs_mesh_from_density against the numpy restatement (tests/marching_cubes_ref.py) bit for bit -- vertices, indices, 1-ring sums and
normals -- on every row of the case table, a random lattice, analytic surfaces, the lattice boundary, degenerate fields and the padding; nrs_mesh_extract against the
library's own lattice and network operator; and the Python face.  The library is built with -ffp-contract=off and these kernels hold no fmaf, so float results compare as
uint32 words; only the colour chain's expf / powf get a margin, the one tests/test_gpu_tonemap.py holds the device powf to: |got - ref| <= 2e-6 * max(1, |ref|)."""
import ctypes as C

import numpy as np
import pytest

import marching_cubes_ref as ref

pytestmark = pytest.mark.gpu
F32 = np.float32
UNIT = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


@pytest.fixture(scope="module")
def table(built):
    from nerfshop_amd import _abi
    lib = _abi.load()
    row_len = C.c_uint32()
    assert lib.nrs_marching_cubes_table(None, C.byref(row_len)) == 0
    t = np.zeros((256, row_len.value), np.int8)
    assert lib.nrs_marching_cubes_table(t.ctypes.data, C.byref(row_len)) == 0
    return t


def run(rig, density, res, thresh, box=UNIT):
    """density: flat [x + y * rx + z * rx * ry] -> (Mesh, V, N, S, F)"""
    t = rig.torch.as_tensor(np.ascontiguousarray(density, F32).reshape(res[2], res[1], res[0]), device="cuda:0")
    mesh = rig.rt.mesh_from_density(rig.ctx, t, box[0], box[1], thresh)
    V, N, Cc, S, Fi = mesh.download()
    assert Cc is None and mesh.d_colors is None
    return mesh, V, N, S, Fi


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def assert_equals_restatement(rig, table, density, res, thresh, box=UNIT, nan_ok=False):
    mesh, V, N, S, Fi = run(rig, density, res, thresh, box)
    want = ref.extract(density, res, box[0], box[1], thresh, table)
    assert (mesh.n_verts, mesh.n_verts_padded, mesh.n_tris) == (want["n_verts"], want["n_padded"], want["n_tris"])
    assert np.array_equal(Fi, want["F"])
    for got, exp, what in ((V, want["V"], "V"), (S, want["S"], "S"), (N, want["N"], "N")):
        if nan_ok:
            np.testing.assert_array_equal(got, exp, err_msg=what)
        else:
            assert np.array_equal(bits(got), bits(exp)), what
    return mesh, V, N, S, Fi, want


def test_every_table_row_on_the_device(rig, table):
    """the 254 non-trivial masks, each a 2 x 2 x 2 lattice with corner values that are not round: dt is not 1/2"""
    rng = np.random.default_rng(254)
    box = ((-0.25, 0.5, 1.0), (1.75, 1.0, 4.0))
    for mask in range(1, 255):
        above = rng.uniform(0.3, 1.7, 8).astype(F32)
        below = rng.uniform(-1.9, 0.2, 8).astype(F32)
        d = np.zeros(8, F32)
        for c in range(8):
            x, y, z = ref.CORNERS[c]
            d[x + 2 * y + 4 * z] = above[c] if (mask >> c) & 1 else below[c]
        mesh, *_ = assert_equals_restatement(rig, table, d, (2, 2, 2), 0.25, box)
        assert mesh.n_tris == len(ref.table_rows(table)[mask]) and mesh.n_verts == len(ref.crossed_edges(mask))


def on_lattice_boundary(v, res, box=UNIT):
    g = (np.asarray(v, np.float64) - np.array(box[0])) / ((np.array(box[1]) - np.array(box[0])) / np.array(res))
    return any(abs(g[k]) < 1e-4 or abs(g[k] - (res[k] - 1)) < 1e-4 for k in range(3))


def test_random_lattice(rig, table):
    """(17, 9, 6): no axis is a multiple of the wave or of the block; U(-1, 1) against 0.1 puts ambiguous faces everywhere"""
    res = (17, 9, 6)
    d = np.random.default_rng(17096).uniform(-1, 1, res[0] * res[1] * res[2]).astype(F32)
    _, V, N, S, Fi, want = assert_equals_restatement(rig, table, d, res, 0.1)
    _, V2, N2, S2, F2 = run(rig, d, res, 0.1)
    assert np.array_equal(bits(V), bits(V2)) and np.array_equal(bits(N), bits(N2)) and np.array_equal(bits(S), bits(S2)) and np.array_equal(Fi, F2)
    assert want["n_tris"] > 1000
    # every mesh edge off the lattice boundary: exactly two triangles, in opposite directions
    for a, b in ref.boundary_edges(Fi):
        assert on_lattice_boundary(V[a], res) and on_lattice_boundary(V[b], res), (a, b)


def test_more_blocks_than_scan_threads(rig, table):
    """8 x 8 x 4100 points are 1025 blocks of 256: each thread of the one-workgroup scan over the blocks' sums owns a run of two.  Three slabs of U(-1, 1), in the
    first blocks, in the middle and in the last ones, in a field that is below the threshold everywhere else."""
    res = (8, 8, 4100)
    rng = np.random.default_rng(4100)
    d = np.full((res[2], res[1] * res[0]), -0.6, F32)
    for z in (3, 2040, 4090):
        d[z:z + 3] = rng.uniform(-1, 1, (3, res[1] * res[0])).astype(F32)
    mesh, V, *_ = assert_equals_restatement(rig, table, d.reshape(-1), res, 0.1)
    assert mesh.n_verts > 600 and mesh.n_tris > 900
    z = V[:mesh.n_verts, 2] * res[2]
    assert ((z > 2) & (z < 7)).any() and ((z > 2039) & (z < 2044)).any() and ((z > 4089) & (z < 4094)).any()


def lattice_points(res, box=UNIT):
    z, y, x = np.meshgrid(*(np.arange(r, dtype=np.float64) for r in res[::-1]), indexing="ij")
    scale = (np.array(box[1]) - np.array(box[0])) / np.array(res)
    return np.stack([x, y, z], axis=-1).reshape(-1, 3) * scale + np.array(box[0])


@pytest.mark.parametrize("shape", ["sphere", "torus"])
def test_analytic_surfaces(rig, table, shape):
    res = (32, 32, 32)
    p = lattice_points(res) - 0.47   # centre off the lattice
    if shape == "sphere":
        field = 0.31 - np.linalg.norm(p, axis=1)
    else:
        ring = np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2) - 0.27
        field = 0.11 - np.sqrt(ring ** 2 + p[:, 2] ** 2)
    mesh, V, N, S, Fi, _ = assert_equals_restatement(rig, table, field.astype(F32), res, 0.0)
    assert ref.boundary_edges(Fi) == []                                            # closed
    n_edges = len({tuple(sorted(e)) for e in ref.edge_uses(Fi)})
    assert mesh.n_verts - n_edges + mesh.n_tris == (2 if shape == "sphere" else 0)  # Euler characteristic
    q = V[:mesh.n_verts].astype(np.float64) - 0.47
    if shape == "sphere":
        outward = q
    else:
        r = np.sqrt(q[:, 0] ** 2 + q[:, 1] ** 2)
        outward = q - np.stack([q[:, 0] / r, q[:, 1] / r, np.zeros_like(r)], axis=1) * 0.27
    assert ((N[:mesh.n_verts].astype(np.float64) * outward).sum(axis=1) > 0).all()   # out of the dense side
    assert (S[:mesh.n_verts, 3] >= 6).all() and not V[mesh.n_verts:].any()


def test_surface_leaving_the_box(rig, table):
    res = (16, 16, 16)
    p = lattice_points(res) - np.array([0.9, 0.5, 0.1])
    field = (0.42 - np.linalg.norm(p, axis=1)).astype(F32)   # a sphere cut by three sides of the lattice
    _, V, _, _, Fi, want = assert_equals_restatement(rig, table, field, res, 0.0)
    edges = ref.boundary_edges(Fi)
    assert len(edges) > 10
    for a, b in edges:
        assert on_lattice_boundary(V[a], res) and on_lattice_boundary(V[b], res)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_slab_in_the_last_layer(rig, table, axis):
    """a field that changes side only between the last two layers of one axis: the `< res - 1` guards of vertices and cells"""
    res = (16, 16, 16)
    idx = np.indices(res[::-1])[2 - axis].reshape(-1)
    field = np.where(idx == res[axis] - 1, 1.0, -0.6).astype(F32)
    mesh, V, *_ = assert_equals_restatement(rig, table, field, res, 0.0)
    assert mesh.n_verts == 256 and mesh.n_tris == 2 * 15 * 15
    assert np.allclose(V[:256, axis], (res[axis] - 2 + 0.375) / res[axis])


def test_degenerate_fields(rig, table):
    res = (16, 16, 16)
    for value in (-1.0, 3.0):   # all below, all above
        mesh, V, N, S, Fi = run(rig, np.full(16 ** 3, value, F32), res, 0.5)
        assert (mesh.n_verts, mesh.n_verts_padded, mesh.n_tris) == (0, 0, 0) and mesh.h
        assert V.shape == (0, 3) and Fi.shape == (0, 3)
        assert rig.ctx.lib.nrs_mesh_download(mesh.h, None, None, None, None, None) == 0
        assert rig.ctx.lib.nrs_mesh_download(mesh.h, None, None, np.zeros(3, F32).ctypes.data, None, None) == -5   # no colours on such a mesh: NRS_ERR_STATE
    # NaN and the mask value of nrs_density_on_grid next to the surface
    p = lattice_points(res) - 0.5
    field = (0.3 - np.linalg.norm(p, axis=1)).astype(F32)
    near = np.flatnonzero(np.abs(field) < 0.05)
    field[near[::5]] = np.nan
    field[near[1::5]] = -10000.0
    assert_equals_restatement(rig, table, field, res, 0.0, nan_ok=True)
    # a value exactly equal to thresh is outside: one point above, its six neighbours at thresh
    field = np.full(16 ** 3, 0.5, F32)
    field[5 + 16 * 6 + 256 * 7] = 1.0
    mesh, *_ = assert_equals_restatement(rig, table, field, res, 0.5)
    assert (mesh.n_verts, mesh.n_tris) == (6, 8)
    field[5 + 16 * 6 + 256 * 7] = 0.5
    assert run(rig, field, res, 0.5)[0].n_verts == 0


def planted_field(n_verts):
    """a (rx, 2, 2) lattice with exactly n_verts crossings: a lone corner point of the lattice crosses its 3 edges, a change of side between two whole y-z sheets crosses 4"""
    corners = next(c for c in range(4) if (n_verts - 3 * c) % 4 == 0 and n_verts >= 3 * c)
    sheets = (n_verts - 3 * corners) // 4
    rx = sheets + 6
    f = np.full((2, 2, rx), -1.0, F32)
    for k in range(sheets):          # columns 3 .. 2 + sheets alternate, the rest of the lattice keeps the last column's side
        f[:, :, 3 + k:] = 1.0 if k % 2 == 0 else -1.0
    if corners >= 1:
        f[0, 0, 0] = 1.0
    if corners >= 2:
        f[1, 1, 0] = 1.0
    if corners >= 3:
        f[0, 0, rx - 1] = -f[0, 0, rx - 1]
    return f.reshape(-1), (rx, 2, 2)


@pytest.mark.parametrize("n_verts", [3, 127, 128, 129])
def test_padding(rig, table, n_verts):
    """n_verts = 3 stands for "one": a lattice with every axis >= 2 has no edge whose removal separates it, so no field crosses fewer than 3 lattice edges"""
    field, res = planted_field(n_verts)
    mesh, V, N, S, Fi, want = assert_equals_restatement(rig, table, field, res, 0.0)
    assert mesh.n_verts == n_verts and mesh.n_verts_padded == (n_verts + 127) // 128 * 128
    assert V.shape[0] == mesh.n_verts_padded and V[:n_verts].any(axis=1).all()
    assert not V[n_verts:].any() and not N[n_verts:].any() and not S[n_verts:].any()


# ---- nrs_mesh_extract on the synthetic model whose geometry sits in the network ---------------------------------------------------------------------------------------
def srgb_margin(got, want):
    return np.abs(got.astype(np.float64) - want) <= 2e-6 * np.maximum(1.0, np.abs(want))


def color_chain(raw, activation, linear_colors):
    """network_to_rgb (float64 where it takes expf) then linear_to_srgb (common_device.cuh:55-61, the pow in float64) -> (values, exact)"""
    from nerfshop_amd import _abi
    raw = raw.astype(F32)
    exact = activation in (_abi.ACT_NONE, _abi.ACT_RELU) and not linear_colors
    if activation == _abi.ACT_RELU:
        c = np.maximum(raw, F32(0)).astype(np.float64)
    elif activation == _abi.ACT_LOGISTIC:
        c = 1.0 / (1.0 + np.exp(-raw.astype(np.float64)))
    elif activation == _abi.ACT_EXPONENTIAL:
        c = np.exp(np.clip(raw, -10, 10).astype(np.float64))
    else:
        c = raw.astype(np.float64)
    if linear_colors:
        c32 = c.astype(F32)
        c = np.where(c32 < F32(0.0031308), (F32(12.92) * c32).astype(np.float64), 1.055 * np.power(c32.astype(np.float64), np.float64(F32(0.41666))) - 0.055)
    return c, exact


def color_inputs(V, aabb_min, aabb_max):
    """generate_nerf_network_inputs_from_positions (testbed_nerf.cu:608-613) in float32"""
    V = V.astype(F32)
    d = V - F32(0.5)
    sq = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    with np.errstate(all="ignore"):
        d = np.where(sq[:, None] > 0, d / np.sqrt(sq)[:, None], d).astype(F32)
    mn, mx = np.asarray(aabb_min, F32), np.asarray(aabb_max, F32)
    out = np.zeros((V.shape[0], 7), F32)
    out[:, :3] = (V - mn) / (mx - mn)
    min_step = F32(np.sqrt(F32(3.0))) / F32(1024.0)
    out[:, 3] = (min_step - min_step) / (min_step * F32(16) - min_step)   # warp_dt(MIN_CONE_STEPSIZE)
    out[:, 4:] = (d + F32(1.0)) * F32(0.5)
    return out


def check_extract(rig, testbed, linear_colors):
    torch, lib = rig.torch, rig.ctx.lib
    net = testbed.nerf_network
    box = ((0.05, 0.1, 0.0), (0.95, 1.0, 0.9))
    lattice = testbed.get_density_on_grid((32, 32, 32), box[0], box[1], mask_with_density_grid=False)
    values = lattice.cpu().numpy()
    thresh = float((np.float64(values.min()) + np.float64(values.max())) / 2)   # a surface certainly exists between the extremes
    testbed.linear_colors = linear_colors
    assert testbed.marching_cubes((30, 17, 32), box, thresh, mask_with_density_grid=False) == testbed.mesh.n_tris > 100   # rounded up to (32, 32, 32)
    mesh = testbed.mesh
    V, N, Cc, S, Fi = mesh.download()
    own = rig.rt.mesh_from_density(rig.ctx, lattice, box[0], box[1], thresh)
    V2, N2, _, S2, F2 = own.download()
    assert mesh.n_verts == own.n_verts and mesh.n_verts_padded == own.n_verts_padded
    assert np.array_equal(bits(V), bits(V2)) and np.array_equal(bits(N), bits(N2)) and np.array_equal(bits(S), bits(S2)) and np.array_equal(Fi, F2)
    # the colour inputs, read back
    coords = torch.zeros((mesh.n_verts_padded, 7), dtype=torch.float32, device="cuda:0")
    assert lib.nrs_mesh_color_inputs(net.h, None, mesh.h, coords.data_ptr()) == 0
    torch.cuda.synchronize()
    want_in = color_inputs(V, testbed.desc.aabb_min, testbed.desc.aabb_max)
    assert np.array_equal(bits(coords.cpu().numpy()), bits(want_in))
    # the colours: the activation chain on the library's own network output for those inputs
    out = torch.zeros((mesh.n_verts_padded, 16), dtype=torch.float16, device="cuda:0")
    net.inference_mixed_precision(None, coords, out)
    torch.cuda.synchronize()
    raw = out.cpu().numpy()[:, :3].astype(F32)
    want, exact = color_chain(raw, testbed.desc.rgb_activation, linear_colors)
    assert Cc.shape == (mesh.n_verts_padded, 3) and raw.std() > 0
    if exact:
        assert np.array_equal(bits(Cc), bits(want.astype(F32)))
    else:
        assert srgb_margin(Cc, want).all(), np.abs(Cc - want).max()


@pytest.mark.parametrize("grid_acc,mlp_acc,linear_colors", [(0, 0, False), (1, 1, True), (0, 1, False), (1, 0, True)])
def test_extract_every_numerics(rig_shaped, grid_acc, mlp_acc, linear_colors):
    net = rig_shaped.net
    net.set_numerics(grid_acc, mlp_acc)
    try:
        check_extract(rig_shaped, rig_shaped.testbed, linear_colors)
    finally:
        net.set_numerics(0, 0)
        rig_shaped.testbed.linear_colors = False


def test_extract_light_direction_model(rig_shaped):
    from nerfshop_amd import synth
    scene = rig_shaped.scene
    tb = rig_shaped.rt.Testbed(rig_shaped.ctx, scene.desc, 1, n_extra_dims=3)
    tb.nerf_network.set_params(synth.make_light_params(scene.desc, sigma_raw=synth.default_sigma_raw(1), shaped=True))
    tb.nerf_network.set_light_dir((0.3, -0.8, 0.5))
    check_extract(rig_shaped, tb, False)
    first = tb.mesh.download()[2]
    tb.nerf_network.set_light_dir((-0.6, 0.1, 0.7))   # the same mesh under another light: other colours
    check_extract(rig_shaped, tb, False)
    assert not np.array_equal(first, tb.mesh.download()[2])


def test_python_face(rig_shaped, tmp_path):
    tb = rig_shaped.testbed
    rig_shaped.net.set_density_grid(rig_shaped.scene.grid)   # the mask of get_density_on_grid needs the float grid (the rig sets the bitfield this grid gives)
    assert tb.get_marching_cubes_res(256, (0, 0, 0), (1, 0.5, 0.3)) == ref.marching_cubes_res(256, (0, 0, 0), (1, 0.5, 0.3))
    box = ((0.05, 0.1, 0.0), (0.95, 1.0, 0.9))
    values = tb.get_density_on_grid((32, 32, 32), box[0], box[1], mask_with_density_grid=True).cpu().numpy()
    thresh = float((np.float64(values[values > -10000].min()) + np.float64(values.max())) / 2)
    m = tb.compute_marching_cubes_mesh((32, 32, 32), box, thresh)
    n, t = tb.mesh.n_verts_padded, tb.mesh.n_tris
    assert n % 128 == 0 and n > 0 and t > 0
    assert m["V"].shape == m["N"].shape == m["C"].shape == (n, 3) and m["F"].shape == (t, 3)
    assert m["V"].dtype == m["N"].dtype == m["C"].dtype == np.float32 and m["F"].dtype == np.int32
    lengths = np.linalg.norm(m["N"][:tb.mesh.n_verts].astype(np.float64), axis=1)
    assert np.abs(lengths - 1).max() < 1e-6 and not m["N"][tb.mesh.n_verts:].any()
    assert m["F"].min() >= 0 and m["F"].max() < tb.mesh.n_verts
    path = tmp_path / "mesh.ply"
    tb.dataset_scale = 0.33
    try:
        tb.compute_and_save_marching_cubes_mesh(str(path), (32, 32, 32), box, thresh, dataset_offset=(0.5, 0.5, 0.5))
    finally:
        tb.dataset_scale = 1.0
    V, N, Cc, S, Fi = tb.mesh.download()
    text = path.read_text()
    assert text == ref.ply_text(V, N, Cc, Fi, 0.33, (0.5, 0.5, 0.5))
    pv, pn, pc, pf = ref.parse_ply(text)
    assert np.array_equal(pf[:, ::-1], m["F"]) and np.abs(pv - (m["V"].astype(np.float64) - 0.5) / np.float64(np.float32(0.33))).max() < 1e-5
    assert np.abs(pn - m["N"]).max() < 1e-3 and np.abs(pc.astype(np.float64) - np.clip(m["C"] * 255.0, 0, 255)).max() <= 1.0
    with pytest.raises(rig_shaped.rt.NrsError, match="unwrap"):
        tb.compute_and_save_marching_cubes_mesh(str(path), 32, box, thresh, unwrap_it=True)
    # an empty aabb means the render box
    assert tb.marching_cubes(16, None, thresh) == tb.mesh.n_tris
