"""The selection tool on an MI355X: nrs_bitfield_morph against its host twin and the numpy reference of tests/selection_ref.py bit for bit, dilate / erode on a selection
handle, and nrs_selection_fine_mesh against nrs_mesh_from_density and tests/marching_cubes_ref.py on the lattice that selection_ref builds.  Everything compares exactly:
bits, cell lists, and float arrays as uint32 words (the lattice holds 0.0 and 1.0 and the mesh code is the one tests/test_gpu_marching_cubes.py pins)."""
import ctypes as C

import numpy as np
import pytest

import marching_cubes_ref as mc
import selection_ref as ref

pytestmark = pytest.mark.gpu
VOL, G = ref.VOL, ref.G
MORPH_CASES = [(op, se, r) for op in (ref.DILATE, ref.ERODE) for se in (ref.CUBE, ref.SPHERE) for r in (1, 2, 3)]


def scribble(w, h, n, seed):
    """a few strokes across the object plus stray pixels (background, image border)"""
    rng = np.random.default_rng(seed)
    t = rng.uniform(0, 1, size=n)
    px = np.stack([(0.5 + 0.28 * np.cos(7 * t) * t) * w, (0.5 + 0.28 * np.sin(5 * t) * t) * h], 1).astype(np.int32)
    px[:4] = [[0, 0], [w - 1, h - 1], [w // 2, h // 2], [w // 2, 0]]
    return px


def cell(x, y, z, level=0):
    return level * VOL + int(ref.morton(x, y, z))


def idle(rig):
    return rig.torch.cuda.current_stream().query()


@pytest.fixture(scope="module")
def table(built):
    from nerfshop_amd import _abi
    lib = _abi.load()
    row_len = C.c_uint32()
    assert lib.nrs_marching_cubes_table(None, C.byref(row_len)) == 0
    t = np.zeros((256, row_len.value), np.int8)
    assert lib.nrs_marching_cubes_table(t.ctypes.data, C.byref(row_len)) == 0
    return t


def device_morph(rig, bits, level, op, se, r):
    d_in = rig.torch.as_tensor(bits, device="cuda:0")
    d_out = rig.torch.full_like(d_in, 0x5A)                  # the call leaves no byte as it found it
    rig.rt.bitfield_morph(rig.ctx, d_in, level, op, se, r, out=d_out)
    rig.torch.cuda.synchronize()
    assert rig.torch.equal(d_in.cpu(), rig.torch.as_tensor(bits))   # the input is only read
    return d_out.cpu().numpy()


@pytest.mark.parametrize("level", [0, 4])
@pytest.mark.parametrize("name", ref.PATTERNS + ("random_inverse",))
def test_morph_device_against_host_twin_and_numpy(rig, name, level):
    bits = ref.grid_to_bits(ref.pattern(name), level)
    other = np.random.default_rng(level).integers(0, 256, ref.BITFIELD_BYTES, dtype=np.uint8)
    other[level * VOL // 8:(level + 1) * VOL // 8] = 0
    bits |= other                                            # every other level of the input holds bits: they are not read, and the output's are zero
    for op, se, r in MORPH_CASES:
        got = device_morph(rig, bits, level, op, se, r)
        want = ref.grid_to_bits(ref.pattern_morph(name, op, se, r), level)
        assert np.array_equal(got, want), (name, level, op, se, r, "numpy")
        assert np.array_equal(got, rig.rt.bitfield_morph_host(bits, level, op, se, r)), (name, level, op, se, r, "host twin")


def radius_ten_probes(name, op):
    """about 500 cells where the verdict is open: near the pattern's set cells (so that about half of them are expected clear after dilation, or set after erosion)
    and within 10 of the faces the pattern reaches"""
    rng = np.random.default_rng(10 + op)
    centre = np.array(ref.BALL_CENTRE)
    probes = []
    lo, hi = (ref.BALL_RADIUS - 12, ref.BALL_RADIUS + 24) if op == ref.DILATE else (2, ref.BALL_RADIUS + 2)
    while len(probes) < 260:                                 # distances from the centre spread evenly over the range in which the operation moves the surface
        d = rng.normal(size=3)
        p = np.rint(centre + d / np.linalg.norm(d) * rng.uniform(lo, hi)).astype(np.int64)
        if (p >= 0).all() and (p < G).all():
            probes.append(p)
    if op == ref.DILATE:                                     # round each lone cell, all of them within 10 of a face
        for c in ref.LONE_CELLS:
            probes.extend(np.clip(np.array(c) + rng.integers(-14, 15, (40, 3)), 0, G - 1))
    else:                                                    # inside the ball where the x = 0 and z = 127 faces cut it: the taps beyond the face do not count
        for axis, face in ((0, 0), (2, G - 1)):
            q = centre + rng.integers(-16, 17, (120, 3))
            q[:, axis] = np.abs(face - rng.integers(0, 11, 120))
            probes.extend(np.clip(q, 0, G - 1))
    return [tuple(int(v) for v in p) for p in probes]


@pytest.mark.parametrize("op,name", [(ref.DILATE, "ball_faces"), (ref.ERODE, "ball_noise")])
def test_radius_ten(rig, op, name):
    """the widest element.  Dilation on a sparse pattern (a ball cut by two faces, a lone cell near each face), erosion on the ball in 2 % noise: the whole level against
    the host twin, the cube also against numpy, and about 500 cells against the tap loop, with both verdicts among them"""
    g = ref.pattern(name)
    level = 2
    bits = ref.grid_to_bits(g, level)
    probes = radius_ten_probes(name, op)
    assert 480 <= len(probes) <= 520
    for se in (ref.CUBE, ref.SPHERE):
        got = device_morph(rig, bits, level, op, se, 10)
        assert np.array_equal(got, rig.rt.bitfield_morph_host(bits, level, op, se, 10)), (op, se)
        grid = ref.bits_to_grid(got, level)
        assert 0 < grid.sum() < ref.VOL // 2
        if se == ref.CUBE:                                   # (numpy's sphere at this radius takes seconds; the tap loop below stands in for it)
            assert np.array_equal(grid, ref.pattern_morph(name, op, se, 10)), (op, se)
        verdicts = [ref.brute_cell(g, x, y, z, op, se, 10) for x, y, z in probes]
        assert 0.2 * len(probes) < sum(verdicts) < 0.8 * len(probes), sum(verdicts)      # neither verdict is the rule
        for (x, y, z), want in zip(probes, verdicts):
            assert grid[x, y, z] == want, (op, se, x, y, z)


def test_morph_arguments_are_checked_before_a_launch(rig):
    lib, torch = rig.ctx.lib, rig.torch
    a = torch.zeros(ref.BITFIELD_BYTES + 32, dtype=torch.uint8, device="cuda:0")
    b = torch.zeros(ref.BITFIELD_BYTES + 32, dtype=torch.uint8, device="cuda:0")
    pa, pb = a.data_ptr(), b.data_ptr()

    def refused(word, *args):
        assert lib.nrs_bitfield_morph(rig.ctx.h, None, *args) == -1
        assert word in lib.nrs_last_error().decode(), lib.nrs_last_error().decode()

    refused("d_in", None, 0, 0, 0, 1, pb)
    refused("d_out", pa, 0, 0, 0, 1, None)
    refused("level", pa, 5, 0, 0, 1, pb)
    refused("op", pa, 0, 2, 0, 1, pb)
    refused("se_type", pa, 0, 0, 2, 1, pb)
    refused("radius", pa, 0, 0, 0, 0, pb)
    refused("radius", pa, 0, 0, 0, 11, pb)
    refused("overlaps", pa, 0, 0, 0, 1, pa + 16)
    refused("d_in is not 16-byte aligned", pa + 4, 0, 0, 0, 1, pb)
    refused("d_out is not 16-byte aligned", pa, 0, 0, 0, 1, pb + 8)
    torch.cuda.synchronize()
    assert not b.any()


# ---- the handle: one grid for the tests below.  A dense ball with a dent and a one-cell hole (what the closing repairs), thin background, and one dense cell on a face ----
@pytest.fixture(scope="module")
def grid(built):
    rng = np.random.default_rng(77)
    g = rng.uniform(0.0, 0.009, ref.CASCADES * VOL).astype(np.float32)
    a = np.arange(G)
    ball = (a[:, None, None] - 40) ** 2 + (a[None, :, None] - 50) ** 2 + (a[None, None, :] - 45) ** 2 <= 6 ** 2
    ball[40, 50, 45] = False                                 # a hole inside
    ball[44:47, 50, 45] = False                              # a dent from the surface
    m = ref.morton_of_grid()
    for level in (0, 1):
        g[level * VOL + m[ball]] = 1.0
    g[cell(0, 100, 100)] = 1.0
    g.setflags(write=False)
    return g


def grown(rig, grid, max_cascade=0, seeds=None, level=0):
    sel = rig.rt.GrowingSelection(rig.ctx, grid, max_cascade)
    sel.reset_growing([cell(38, 50, 45, level)] if seeds is None else seeds, level)
    sel.grow_region(0.01, level, 10000)
    return sel


def level_grid(sel):
    return ref.bits_to_grid(sel.selection_grid_bitfield, sel.growing_level)


def test_dilate_and_erode_on_the_handle(rig, grid):
    sel = grown(rig, grid)
    before = level_grid(sel)
    assert before.sum() > 800 and not before[40, 50, 45]
    sel.dilate()
    assert idle(rig)
    want = ref.dilate(before, ref.CUBE, 2)                   # the handle's defaults: Cube 2, then Sphere 2
    assert np.array_equal(level_grid(sel), want)
    assert np.array_equal(sel.selection_cell_idx, ref.cells_in_loop_order(want, 0))       # rebuilt x outer, y, z inner: no seed, no duplicate left
    assert np.array_equal(sel.selection_points.view(np.uint32), ref.cell_pos(sel.selection_cell_idx).view(np.uint32))
    sel.erode()
    assert idle(rig)
    want = ref.erode(want, ref.SPHERE, 2)
    assert np.array_equal(level_grid(sel), want) and np.array_equal(sel.selection_cell_idx, ref.cells_in_loop_order(want, 0))
    assert want[40, 50, 45] and want[45, 50, 45]             # the closing filled the hole and the dent
    assert not sel.performed_closing                         # dilate / erode by hand do not touch the flag
    sel.set_structuring_elements((ref.SPHERE, 3), (ref.CUBE, 1))
    sel.erode()
    want = ref.erode(want, ref.CUBE, 1)
    sel.dilate()
    want = ref.dilate(want, ref.SPHERE, 3)
    assert np.array_equal(level_grid(sel), want) and np.array_equal(sel.selection_cell_idx, ref.cells_in_loop_order(want, 0))
    other = np.delete(sel.selection_grid_bitfield.reshape(ref.CASCADES, -1), 0, axis=0)
    assert not other.any()


def assert_mesh_of_lattice(rig, table, mesh, lattice, level):
    """bit-equal to nrs_mesh_from_density of the same lattice (vertices, triangles, both 1-ring sums) and to the numpy restatement (vertices, triangles)"""
    box = ref.level_box(level)
    twin = rig.rt.mesh_from_density(rig.ctx, rig.torch.as_tensor(lattice, device="cuda:0"), box[0], box[1], 0.5)
    V, N, Cc, S, F = mesh.download()
    V2, N2, _, S2, F2 = twin.download()
    assert Cc is None
    assert (mesh.n_verts, mesh.n_verts_padded, mesh.n_tris) == (twin.n_verts, twin.n_verts_padded, twin.n_tris)
    u = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    assert np.array_equal(F, F2) and np.array_equal(u(V), u(V2)) and np.array_equal(u(S), u(S2)) and np.array_equal(u(N), u(N2))
    want = mc.extract(lattice.reshape(-1), (G, G, G), box[0], box[1], 0.5, table)
    assert (mesh.n_verts, mesh.n_verts_padded, mesh.n_tris) == (want["n_verts"], want["n_padded"], want["n_tris"])
    assert np.array_equal(F, want["F"]) and np.array_equal(u(V), u(want["V"]))
    assert mc.boundary_edges(F) == []
    return V, F


def test_fine_mesh_with_the_closing(rig, grid, table):
    sel = grown(rig, grid)
    before = level_grid(sel)
    mesh = sel.extract_fine_mesh()
    assert idle(rig) and sel.performed_closing
    closed = ref.erode(ref.dilate(before, ref.CUBE, 2), ref.SPHERE, 2)
    assert np.array_equal(level_grid(sel), closed) and np.array_equal(sel.selection_cell_idx, ref.cells_in_loop_order(closed, 0))
    lattice = ref.lattice(sel.selection_cell_idx, 0)
    assert lattice.sum() == closed.sum() > before.sum()
    assert_mesh_of_lattice(rig, table, mesh, lattice, 0)
    n_tris = mesh.n_tris
    # a second call does not close again: closing is not idempotent here in general, so compare with what one closing gave
    sel.set_structuring_elements((ref.CUBE, 3), (ref.SPHERE, 1))      # (would change the result if it ran)
    mesh = sel.extract_fine_mesh()
    assert np.array_equal(level_grid(sel), closed) and mesh.n_tris == n_tris
    # a grow in between clears the flag: the next call closes again, with the elements now set
    sel.reset_growing([cell(38, 50, 45)], 0)
    sel.grow_region(0.01, 0, 10000)
    assert not sel.performed_closing and np.array_equal(level_grid(sel), before)
    mesh = sel.extract_fine_mesh()
    again = ref.erode(ref.dilate(before, ref.CUBE, 3), ref.SPHERE, 1)
    assert sel.performed_closing and np.array_equal(level_grid(sel), again) and not np.array_equal(again, closed)
    assert_mesh_of_lattice(rig, table, mesh, ref.lattice(sel.selection_cell_idx, 0), 0)


def test_fine_mesh_without_morphology_follows_the_list(rig, grid, table):
    """L, not S: a seed that failed the density test contributes its cube; a cell on the grid's shell contributes nothing"""
    failed, on_face = cell(90, 20, 20), cell(0, 100, 100)
    assert grid[failed] < 0.01 and grid[on_face] >= 0.01
    sel = grown(rig, grid, seeds=[cell(38, 50, 45), failed, on_face])
    sel.use_morphological = False
    L = sel.selection_cell_idx
    S = level_grid(sel)
    assert failed in L and not S[90, 20, 20] and S[0, 100, 100]      # (max_cascade 0: the face cell is accepted where it is)
    mesh = sel.extract_fine_mesh()
    assert idle(rig) and not sel.performed_closing and np.array_equal(sel.selection_cell_idx, L)
    lattice = ref.lattice(L, 0)
    assert lattice[20, 20, 90] == 1.0 and lattice[100, 100, 0] == 0.0 and lattice.sum() == S.sum() + 1 - 1
    V, F = assert_mesh_of_lattice(rig, table, mesh, lattice, 0)
    centre = ref.cell_pos([failed])[0] - np.float32(0.5 / G)          # lattice point (90, 20, 20) of the box [0, 1]^3
    near = np.abs(V[:mesh.n_verts] - centre).max(axis=1) < 0.6 / G
    assert near.sum() == 6                                            # the lone cell's octahedron
    assert not (np.abs(V[:mesh.n_verts] - np.array([0.0, 100 / G, 100 / G], np.float32)).max(axis=1) < 1.5 / G).any()


def test_fine_mesh_at_a_higher_level(rig, grid, table):
    """a selection that was upscaled: the box is 0.5 +- 0.5 * 2^g, and only the cells of level g count"""
    sel = grown(rig, grid, max_cascade=1, seeds=[cell(38, 50, 45, 1)], level=1)
    assert sel.growing_level == 1
    mesh = sel.extract_fine_mesh()
    assert idle(rig)
    lattice = ref.lattice(sel.selection_cell_idx, 1)
    V, _ = assert_mesh_of_lattice(rig, table, mesh, lattice, 1)
    assert mesh.n_tris > 0 and V[:mesh.n_verts].min() > -0.5 and V[:mesh.n_verts].max() < 1.5 and V[:mesh.n_verts].min() < 0.5


def test_scribble_to_selection_mesh(rig, table):
    """project_selection_pixels -> reset_growing -> grow_region with the reference's defaults -> extract_fine_mesh on the synthetic scene"""
    scene = rig.scene
    rig.use_edit(False)
    tb = rig.rt.Testbed(rig.ctx, scene.desc, 1)
    tb.nerf_network.set_params(scene.params)
    tb.nerf_network.set_density_grid(scene.grid)
    w, h = 640, 360
    px = scribble(w, h, 400, 11)
    _, (cells, _, level) = tb.project_selection_pixels(scene.params_for(w, h, 50.0), px)
    assert len(cells) > 50
    sel = tb.growing_selection(max_cascade=0)
    sel.reset_growing(cells, level)
    assert 0 < sel.grow_region() <= 10000 and sel.growing_level == level
    mesh = sel.extract_fine_mesh()
    assert idle(rig) and sel.performed_closing
    V, _, _, _, F = mesh.download()
    assert mesh.n_tris > 0 and mc.boundary_edges(F) == []
    lo, hi = ref.level_box(level)
    assert (V[:mesh.n_verts] > lo[0]).all() and (V[:mesh.n_verts] < hi[0]).all()
    assert_mesh_of_lattice(rig, table, mesh, ref.lattice(sel.selection_cell_idx, level), level)
