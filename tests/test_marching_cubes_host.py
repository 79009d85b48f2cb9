"""CPU-only: the host half of mesh extraction.  The exports exist; the case table the library generates equals the one an independent Python generator
(tests/marching_cubes_ref.py) makes from the rule of DESIGN.md section 2, and has the rule's properties mask by mask and across every pair of face-adjacent cells;
nrs_marching_cubes_res and nrs_mesh_write agree with float32 restatements; every refusal of nrs_mesh_from_density that needs no device names its argument."""
import ctypes as C
import itertools
import math
import os

import numpy as np
import pytest

import marching_cubes_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nrs_marching_cubes_res", "nrs_marching_cubes_table", "nrs_mesh_write", "nrs_mesh_from_density", "nrs_mesh_extract", "nrs_mesh_color_inputs", "nrs_mesh_counts",
         "nrs_mesh_device", "nrs_mesh_download", "nrs_mesh_destroy")


@pytest.fixture(scope="module")
def lib(built):
    from nerfshop_amd import _abi
    return _abi.load()


@pytest.fixture(scope="module")
def table(lib):
    row_len = C.c_uint32()
    assert lib.nrs_marching_cubes_table(None, C.byref(row_len)) == 0
    t = np.full((256, row_len.value), 99, np.int8)
    assert lib.nrs_marching_cubes_table(t.ctypes.data, C.byref(row_len)) == 0
    return t


def test_mesh_entry_points_are_exported(lib):
    from nerfshop_amd import _abi
    header = open(os.path.join(ROOT, "include", "nrs.h")).read()
    for name in NAMES:
        assert name in _abi.EXPORTS and hasattr(lib, name) and f"{name}(" in header, name
    assert "#define NRS_ABI_VERSION 3 " in header and lib.nrs_abi_version() == 3


def test_table_equals_the_regenerated_one(table):
    mine, row_len = ref.generate_table()
    assert table.shape == (256, row_len)   # the row length is what the generator finds, not an assumed 16
    assert np.array_equal(table, mine)


def _outward(mask, tri):
    """sum over the triangle's three crossed edges of (unset end - set end): the direction out of the dense side at this triangle"""
    g = np.zeros(3)
    for e in tri:
        a, b = ref.EDGES[e]
        s, u = (a, b) if (mask >> a) & 1 else (b, a)
        g += ref.CORNERS[u] - ref.CORNERS[s]
    return g


def test_table_properties_of_every_mask(table):
    rows = ref.table_rows(table)
    assert rows[0] == [] and rows[255] == []
    for mask in range(256):
        listed = sorted({e for tri in rows[mask] for e in tri})
        assert listed == ref.crossed_edges(mask), mask      # every listed edge is crossed, every crossed edge is listed
        assert (table[mask, 3 * len(rows[mask]):] == -1).all()
        for tri in rows[mask]:
            # corner values 0 / 1 and thresh 0.5 put every vertex on its edge's midpoint
            pa, pb, pc = (ref.edge_midpoint(e) for e in tri)
            n = np.cross(pb - pa, pa - pc)
            assert np.dot(n, n) > 0, (mask, tri)             # not degenerate
            assert np.dot(n, _outward(mask, tri)) > 0, (mask, tri)


def test_loops_are_listed_by_their_lowest_edge_and_fans_avoid_the_faces(table):
    rows = ref.table_rows(table)
    for mask in range(256):
        fans, lowest = [], []
        for tri in rows[mask]:
            if not fans or fans[-1][0][0] != tri[0] or fans[-1][-1][2] != tri[1]:
                fans.append([])
            fans[-1].append(tri)
        for fan in fans:
            loop = [fan[0][0], fan[0][1]] + [t[2] for t in fan]
            lowest.append(min(loop))
            for t in fan[:-1]:   # the fan's inner diagonals (apex, t[2])
                assert not ref.share_a_face(t[0], t[2]), (mask, t)
        assert lowest == sorted(lowest), mask


def test_table_is_consistent_across_every_shared_face(table):
    """all 3 x 4096 pairs of face-adjacent cells: a triangle edge that lies inside the shared face is never used by one triangle only (the classic table fails this)"""
    rows = ref.table_rows(table)
    for axis in range(3):
        step = np.zeros(3, int)
        step[axis] = 1
        high = [c for c in range(8) if ref.CORNERS[c][axis] == 1]
        low = [next(c for c in range(8) if (ref.CORNERS[c] == ref.CORNERS[h] - step).all()) for h in high]
        on_face = {0: {e for e in range(12) if all(ref.CORNERS[c][axis] == 1 for c in ref.EDGES[e])},    # cell A's edges on the shared face
                   1: {e for e in range(12) if all(ref.CORNERS[c][axis] == 0 for c in ref.EDGES[e])}}   # cell B's
        for bits in itertools.product(range(2), repeat=12):
            # cell A is the lower cell; cell B sits on its high face: B's low corners are A's high corners
            a_bits, shared, b_high = bits[:4], bits[4:8], bits[8:]
            mask_a = sum(v << c for v, c in zip(a_bits, low)) | sum(v << c for v, c in zip(shared, high))
            mask_b = sum(v << c for v, c in zip(shared, low)) | sum(v << c for v, c in zip(b_high, high))
            uses = {}
            for which, mask in ((0, mask_a), (1, mask_b)):
                for tri in rows[mask]:
                    for e0, e1 in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])):
                        if e0 in on_face[which] and e1 in on_face[which]:
                            key = frozenset((tuple(ref.edge_midpoint(e0) + which * step), tuple(ref.edge_midpoint(e1) + which * step)))
                            uses[key] = uses.get(key, 0) + 1
            assert all(v == 2 for v in uses.values()), (axis, mask_a, mask_b, uses)   # exactly one triangle from either cell


def test_marching_cubes_res(lib):
    rng = np.random.default_rng(20240611)
    cases = [(256, (0, 0, 0), (1, 1, 1)), (16, (0, 0, 0), (1, 1, 1)), (128, (0, 0, 0), (1, 0.5, 0.25)), (24, (0, 0, 0), (1, 1, 1)), (8, (0, 0, 0), (1, 1, 1)),
             (33, (0, 0, 0), (1, 0.5, 0.5)),     # 16.5 on two axes: the half-way case
             (31, (0, 0, 0), (2, 1, 1)), (1, (0, 0, 0), (1, 1, 1)), (0, (0, 0, 0), (1, 1, 1))]
    for _ in range(200):
        mn = rng.uniform(-2, 2, 3).astype(np.float32)
        mx = mn + rng.uniform(0.01, 4, 3).astype(np.float32)
        cases.append((int(rng.integers(1, 700)), tuple(mn), tuple(mx)))
    for res_1d, mn, mx in cases:
        out = (C.c_uint32 * 3)()
        assert lib.nrs_marching_cubes_res(res_1d, C.byref((C.c_float * 3)(*mn)), C.byref((C.c_float * 3)(*mx)), C.byref(out)) == 0
        assert tuple(out) == ref.marching_cubes_res(res_1d, mn, mx), (res_1d, mn, mx)
        assert all(v % 16 == 0 for v in out)
    out = (C.c_uint32 * 3)()
    assert lib.nrs_marching_cubes_res(64, C.byref((C.c_float * 3)(0, 0, 0)), C.byref((C.c_float * 3)(0, 0, 0)), C.byref(out)) == -1
    assert lib.nrs_marching_cubes_res(64, C.byref((C.c_float * 3)(0, 0, 0)), C.byref((C.c_float * 3)(1, math.nan, 1)), C.byref(out)) == -1


def _small_mesh():
    V = np.array([[0.1, 0.2, 0.3], [1.5, -2.25, 3.125], [0.333333, 0.666667, 1.0], [10.0, 20.0, 30.0], [0.0, 0.0, 0.0]], np.float32)
    N = np.array([[0.0, 0.0, 2.0], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [-3.0, 4.0, 0.0], [1e-3, 0.0, 0.0]], np.float32)   # a zero normal stays zero
    Cc = np.array([[0.0, 0.5, 1.0], [1.5, -0.25, 0.999], [0.2, 0.4, 0.6], [0.00390625, 0.9961, 1.0001], [0.5, 0.5, 0.5]], np.float32)   # colours outside [0, 1]
    F = np.array([[0, 1, 2], [2, 3, 4], [4, 0, 3]], np.uint32)
    return V, N, Cc, F


@pytest.mark.parametrize("name,text_of", [("mesh.ply", ref.ply_text), ("mesh.obj", ref.obj_text), ("mesh.ply.txt", ref.obj_text), ("dir.ply/mesh", ref.obj_text)])
@pytest.mark.parametrize("scale,offset", [(1.0, (0.0, 0.0, 0.0)), (0.33, (0.5, 0.25, -1.0))])
def test_mesh_write(lib, tmp_path, name, text_of, scale, offset):
    V, N, Cc, F = _small_mesh()
    path = tmp_path / name
    path.parent.mkdir(parents=True, exist_ok=True)
    assert lib.nrs_mesh_write(os.fsencode(str(path)), len(V), V.ctypes.data, N.ctypes.data, Cc.ctypes.data, len(F), F.ctypes.data, scale, C.byref((C.c_float * 3)(*offset))) == 0
    got = path.read_bytes().decode()
    assert got == text_of(V, N, Cc, F, scale, offset)
    if text_of is ref.ply_text:
        assert "3 2 1 0\n" in got and "3 4 3 2\n" in got       # faces in reversed index order
        pv, pn, pc, pf = ref.parse_ply(got)
        assert np.array_equal(pf[:, ::-1], F) and pc[1].tolist() == [255, 0, 254]
    else:
        assert "f 3//3 2//2 1//1\n" in got and "vn 0.00000 0.00000 0.00000\n" in got


def test_mesh_write_refuses_an_unwritable_path_by_name(lib, tmp_path):
    V, N, Cc, F = _small_mesh()
    path = os.fsencode(str(tmp_path / "no_such_directory" / "mesh.ply"))
    assert lib.nrs_mesh_write(path, len(V), V.ctypes.data, N.ctypes.data, Cc.ctypes.data, len(F), F.ctypes.data, 1.0, C.byref((C.c_float * 3)(0, 0, 0))) == -1
    msg = lib.nrs_last_error()
    assert msg.startswith(b"nrs_mesh_write") and b"no_such_directory" in msg
    assert lib.nrs_mesh_write(None, 0, None, None, None, 0, None, 1.0, C.byref((C.c_float * 3)(0, 0, 0))) == -1 and b"path" in lib.nrs_last_error()


def test_from_density_arguments_refused_without_a_device(lib):
    buf = (C.c_float * 16)()   # never dereferenced (nor is the "context"): every call below is refused first
    ptr = C.addressof(buf)
    inf, nan = math.inf, math.nan

    def call(ctx=ptr, res=(8, 8, 8), mn=(0, 0, 0), mx=(1, 1, 1), thresh=2.5, density=ptr, out=True):
        h = C.c_void_p()
        r = lib.nrs_mesh_from_density(ctx, None, C.byref((C.c_uint32 * 3)(*res)) if res else None, C.byref((C.c_float * 3)(*mn)) if mn else None,
                                      C.byref((C.c_float * 3)(*mx)) if mx else None, thresh, density, C.byref(h) if out else None)
        assert h.value is None
        return r

    calls = [(lambda: call(ctx=None), b"ctx"), (lambda: call(res=None), b"res3d"), (lambda: call(mn=None), b"aabb_min"), (lambda: call(mx=None), b"aabb_max"),
             (lambda: call(density=None), b"d_density"), (lambda: call(out=False), b"mesh_out"),
             (lambda: call(res=(1, 8, 8)), b"res3d"), (lambda: call(res=(8, 0, 8)), b"res3d"), (lambda: call(res=(8, 8, 1)), b"res3d"),
             (lambda: call(res=(1024, 1024, 683)), b"2^31"), (lambda: call(res=(65536, 65536, 2)), b"2^31"), (lambda: call(res=(4294967295, 4294967295, 4294967295)), b"2^31"),
             (lambda: call(thresh=nan), b"thresh"), (lambda: call(thresh=inf), b"thresh"), (lambda: call(thresh=-inf), b"thresh"),
             (lambda: call(mn=(0, nan, 0)), b"aabb_min"), (lambda: call(mn=(-inf, 0, 0)), b"aabb_min"), (lambda: call(mx=(1, 1, inf)), b"aabb_max"), (lambda: call(mx=(nan, 1, 1)), b"aabb_max"),
             (lambda: call(mx=(1, 0, 1)), b"aabb_max"), (lambda: call(mn=(0, 0, 2)), b"aabb_max"), (lambda: call(mn=(1, 0, 0)), b"aabb_max")]
    for fn, word in calls:
        assert fn() == -1, word   # NRS_ERR_INVALID_ARG
        msg = lib.nrs_last_error()
        assert word in msg and msg.startswith(b"nrs_mesh_from_density"), msg
    # the largest lattice that passes, 3 * n = 2^31 - 2: 1024 x 1024 x 682 ... is refused no more by the argument check (the next refusal in line would need a device)
    assert 3 * 1024 * 1024 * 683 >= 2 ** 31 > 3 * 1024 * 1024 * 682


def test_extract_and_access_refuse_null_handles(lib):
    h = C.c_void_p()
    res, mn, mx = (C.c_uint32 * 3)(16, 16, 16), (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    assert lib.nrs_mesh_extract(None, None, C.byref(res), C.byref(mn), C.byref(mx), 2.5, 0, 0, C.byref(h)) == -1 and b"model" in lib.nrs_last_error()
    assert lib.nrs_mesh_counts(None, None, None, None) == -1 and b"mesh" in lib.nrs_last_error()
    assert lib.nrs_mesh_device(None, None, None, None, None, None) == -1 and b"mesh" in lib.nrs_last_error()
    assert lib.nrs_mesh_download(None, None, None, None, None, None) == -1 and b"mesh" in lib.nrs_last_error()
    lib.nrs_mesh_destroy(None)


def test_restatement_on_a_random_lattice_is_a_closed_surface(table):
    """the yardstick itself (no library code beyond the table): on the lattice of the GPU test every mesh edge off the lattice boundary has one triangle on either side"""
    rng = np.random.default_rng(17096)
    res = (17, 9, 6)
    d = rng.uniform(-1, 1, res[0] * res[1] * res[2]).astype(np.float32)
    out = ref.extract(d, res, (0, 0, 0), (1, 1, 1), 0.1, table)
    assert out["n_tris"] > 1000
    scale = 1.0 / np.array(res)
    for a, b in ref.boundary_edges(out["F"]):
        for v in (out["V"][a], out["V"][b]):
            g = v / scale
            assert any(abs(g[k]) < 1e-4 or abs(g[k] - (res[k] - 1)) < 1e-4 for k in range(3)), (a, b, g)
