"""The yardstick of the marching-cubes tests: a plain numpy / Python restatement of what include/nrs.h promises for nrs_mesh_from_density, nrs_marching_cubes_res,
nrs_marching_cubes_table and nrs_mesh_write.  Written from the description in the header and DESIGN.md, not from the library's code: the case table is generated here
from the stated rule with geometry (the library hard-wires the cube's faces), vertices are placed with vectorised float32 arithmetic, triangles are walked cell by
cell, and the 1-ring sums are added one triangle after the other in float32.
"""
import itertools

import numpy as np

F32 = np.float32

# the cube: corners 0..3 round the z = 0 face, 4..7 above them; edges 0..3 / 4..7 round those faces, 8..11 in +z from corners 0..3
CORNERS = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)])
EDGES = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]
EDGE_OF = {frozenset(e): k for k, e in enumerate(EDGES)}


def _faces():
    """the six faces, corners counter-clockwise as seen from outside the cube (worked out from the coordinates)"""
    faces = []
    for axis in range(3):
        for side in (0, 1):
            cs = [c for c in range(8) if CORNERS[c][axis] == side]
            centre = CORNERS[cs].mean(axis=0)
            outward = np.zeros(3)
            outward[axis] = 1.0 if side else -1.0
            u = CORNERS[cs[0]] - centre                       # angle round the outward normal, measured from the first corner
            v = np.cross(outward, u)
            cs.sort(key=lambda c: np.arctan2(np.dot(CORNERS[c] - centre, v), np.dot(CORNERS[c] - centre, u)))
            faces.append(cs)
    return faces


FACES = _faces()


def crossed_edges(mask):
    return [k for k, (a, b) in enumerate(EDGES) if ((mask >> a) & 1) != ((mask >> b) & 1)]


def face_segments(mask, face):
    """directed segments (from edge, to edge) of one face: every maximal run of set corners, walking counter-clockwise, is cut off by one segment that
    leads from the edge where the walk leaves the run to the edge where it entered it.  Two set corners on a diagonal are two runs: each is cut off on its own."""
    s = [(mask >> c) & 1 for c in face]
    leave = [EDGE_OF[frozenset((face[i], face[(i + 1) % 4]))] for i in range(4) if s[i] and not s[(i + 1) % 4]]
    enter = {face[(i + 1) % 4]: EDGE_OF[frozenset((face[i], face[(i + 1) % 4]))] for i in range(4) if not s[i] and s[(i + 1) % 4]}
    segs = []
    for i in range(4):
        if s[i] and not s[(i + 1) % 4]:           # the run that ends at corner i: walk back to its first corner
            j = i
            while s[(j - 1) % 4]:
                j -= 1
            segs.append((EDGE_OF[frozenset((face[i], face[(i + 1) % 4]))], enter[face[j % 4]]))
    assert len(segs) == len(leave)
    return segs


def share_a_face(e0, e1):
    corners = set(EDGES[e0]) | set(EDGES[e1])
    return any(corners <= set(face) for face in FACES)


def mask_triangles(mask):
    """the triangles of a mask as edge-number triples: loops in order of their lowest edge; a loop is walked from that edge and fanned from the first edge
    on the walk whose fan has no diagonal inside a cube face (a diagonal there would lie in the neighbour cell's face too: an edge with four triangles)"""
    nxt = {}
    for face in FACES:
        for a, b in face_segments(mask, face):
            assert a not in nxt
            nxt[a] = b
    assert sorted(nxt) == crossed_edges(mask) and sorted(nxt.values()) == sorted(nxt)
    tris, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start and len(loop) >= 3
        k = len(loop)
        apex = next(s for s in range(k) if not any(share_a_face(loop[s], loop[(s + i) % k]) for i in range(2, k - 1)))
        loop = loop[apex:] + loop[:apex]
        tris += [(loop[0], loop[i], loop[i + 1]) for i in range(1, k - 1)]
    return tris


def generate_table():
    """(table [256, row_len] int8 terminated by -1, row_len): row_len is what the longest row needs"""
    rows = [[e for t in mask_triangles(m) for e in t] for m in range(256)]
    row_len = max(len(r) for r in rows) + 1
    table = np.full((256, row_len), -1, np.int8)
    for m, r in enumerate(rows):
        table[m, :len(r)] = r
    return table, row_len


def table_rows(table):
    """[256] lists of edge triples from an exported table"""
    out = []
    for m in range(256):
        row = [int(v) for v in table[m]]
        n = row.index(-1)
        assert n % 3 == 0
        out.append([tuple(row[i:i + 3]) for i in range(0, n, 3)])
    return out


def edge_midpoint(e):
    a, b = EDGES[e]
    return (CORNERS[a] + CORNERS[b]) / 2.0


def marching_cubes_res(res_1d, aabb_min, aabb_max):
    d = np.asarray(aabb_max, F32) - np.asarray(aabb_min, F32)
    scale = F32(res_1d) / d.max()
    r = (d * scale + F32(0.5)).astype(np.int32)
    return tuple(int((int(v) + 15) // 16 * 16) for v in r)


# (point offset in x, y, z; axis) of the lattice edge behind each of the cube's 12 edges
EDGE_SITE = [((0, 0, 0), 0), ((1, 0, 0), 1), ((0, 1, 0), 0), ((0, 0, 0), 1), ((0, 0, 1), 0), ((1, 0, 1), 1), ((0, 1, 1), 0), ((0, 0, 1), 1),
             ((0, 0, 0), 2), ((1, 0, 0), 2), ((1, 1, 0), 2), ((0, 1, 0), 2)]


def extract(density, res3d, aabb_min, aabb_max, thresh, table):
    """density: flat float32 [x + y * rx + z * rx * ry].  Returns dict(n_verts, n_padded, n_tris, V [n_padded, 3], F [n_tris, 3] uint32, S [n_padded, 4], N [n_padded, 3])."""
    rx, ry, rz = (int(v) for v in res3d)
    d = np.asarray(density, F32).reshape(rz, ry, rx)
    thresh = F32(thresh)
    mn = np.asarray(aabb_min, F32)
    scale = (np.asarray(aabb_max, F32) - mn) / np.array([rx, ry, rz], F32)
    with np.errstate(invalid="ignore"):
        inside = d > thresh
    # vertices: ascending (cell index, axis)
    cross = np.zeros((rz, ry, rx, 3), bool)
    cross[:, :, :-1, 0] = inside[:, :, :-1] != inside[:, :, 1:]
    cross[:, :-1, :, 1] = inside[:, :-1, :] != inside[:, 1:, :]
    cross[:-1, :, :, 2] = inside[:-1, :, :] != inside[1:, :, :]
    flat = cross.reshape(-1)
    n_verts = int(flat.sum())
    n_padded = (n_verts + 127) & ~127
    vidx = np.full(flat.shape, -1, np.int64)
    vidx[flat] = np.arange(n_verts)
    vidx = vidx.reshape(rz, ry, rx, 3)
    zz, yy, xx, aa = np.nonzero(cross)
    f0 = d[zz, yy, xx]
    f1 = d[zz + (aa == 2), yy + (aa == 1), xx + (aa == 0)]
    with np.errstate(all="ignore"):
        dt = (thresh - f0) / (f1 - f0)
    p = np.stack([xx, yy, zz], axis=1).astype(F32)
    p[np.arange(n_verts), aa] = p[np.arange(n_verts), aa] + dt
    V = np.zeros((n_padded, 3), F32)
    with np.errstate(all="ignore"):
        V[:n_verts] = p * scale + mn
    # triangles: ascending cell index, table order inside a cell
    rows = table_rows(table)
    m = np.zeros((rz - 1, ry - 1, rx - 1), np.int32)
    for c in range(8):
        ox, oy, oz = CORNERS[c]
        m |= inside[oz:oz + rz - 1, oy:oy + ry - 1, ox:ox + rx - 1].astype(np.int32) << c
    F = []
    for z, y, x in zip(*np.nonzero((m != 0) & (m != 255))):
        for tri in rows[m[z, y, x]]:
            ids = []
            for e in tri:
                (ox, oy, oz), a = EDGE_SITE[e]
                v = vidx[z + oz, y + oy, x + ox, a]
                assert v >= 0
                ids.append(v)
            F.append(ids)
    F = np.array(F, np.uint32).reshape(-1, 3)
    # 1-ring: sequential float32 sums in ascending triangle order
    S = np.zeros((n_padded, 4), F32)
    N = np.zeros((n_padded, 3), F32)
    two = F32(2.0)
    with np.errstate(all="ignore"):
        for ia, ib, ic in F:
            pa, pb, pc = V[ia], V[ib], V[ic]
            S[ia, :3] += pb + pc
            S[ib, :3] += pa + pc
            S[ic, :3] += pb + pa
            S[ia, 3] += two
            S[ib, 3] += two
            S[ic, 3] += two
            u, w = pb - pa, pa - pc
            n = np.array([u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]], F32)
            N[ia] += n
            N[ib] += n
            N[ic] += n
    return {"n_verts": n_verts, "n_padded": n_padded, "n_tris": len(F), "V": V, "F": F, "S": S, "N": N}


def edge_uses(F):
    """{(a, b) directed: count} over the triangles' three directed edges"""
    uses = {}
    for a, b, c in np.asarray(F).tolist():
        for e in ((a, b), (b, c), (c, a)):
            uses[e] = uses.get(e, 0) + 1
    return uses


def boundary_edges(F):
    """undirected edges that are not used exactly once in each direction"""
    uses = edge_uses(F)
    return sorted({tuple(sorted(e)) for e in uses if uses[e] != 1 or uses.get((e[1], e[0]), 0) != 1})


# ---- the files of nrs_mesh_write ------------------------------------------------------------------------------------------------------------------------------
def _normalized(n):
    n = np.asarray(n, F32)
    sq = F32(n[0] * n[0]) + F32(n[1] * n[1]) + F32(n[2] * n[2])
    with np.errstate(all="ignore"):
        return n / np.sqrt(sq, dtype=F32) if sq > 0 else n


def _c(fmt, *vals):
    """C's printf on floats promoted to double"""
    return fmt % tuple(float(v) if isinstance(v, (np.floating, float)) else int(v) for v in vals)


def _clamp(v, lo, hi):
    v = F32(v)
    return F32(lo) if v < lo else (F32(hi) if v > hi else v)


def ply_text(V, N, C, F, scale=1.0, offset=(0, 0, 0)):
    V, N, C = np.asarray(V, F32), np.asarray(N, F32), np.asarray(C, F32)
    F = np.asarray(F).reshape(-1, 3)
    out = ["ply\nformat ascii 1.0\ncomment output from https://github.com/NVlabs/instant-ngp\n"
           "element vertex %u\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n"
           "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face %u\nproperty list uchar int vertex_index\nend_header\n" % (len(V), len(F))]
    off = np.asarray(offset, F32)
    for v, n, c in zip(V, N, C):
        p = (v - off) / F32(scale)
        n = _normalized(n)
        c8 = [int(_clamp(F32(x) * F32(255.0), 0.0, 255.0)) for x in c]
        out.append(_c("%0.5f %0.5f %0.5f %0.3f %0.3f %0.3f %d %d %d\n", p[0], p[1], p[2], n[0], n[1], n[2], *c8))
    for a, b, c in F.tolist():
        out.append("3 %d %d %d\n" % (c, b, a))
    return "".join(out)


def obj_text(V, N, C, F, scale=1.0, offset=(0, 0, 0)):
    V, N, C = np.asarray(V, F32), np.asarray(N, F32), np.asarray(C, F32)
    F = np.asarray(F).reshape(-1, 3)
    off = np.asarray(offset, F32)
    out = []
    for v, c in zip(V, C):
        p = (v - off) / F32(scale)
        out.append(_c("v %0.5f %0.5f %0.5f %0.3f %0.3f %0.3f\n", p[0], p[1], p[2], _clamp(c[0], 0.0, 1.0), _clamp(c[1], 0.0, 1.0), _clamp(c[2], 0.0, 1.0)))
    for n in N:
        n = _normalized(n)
        out.append(_c("vn %0.5f %0.5f %0.5f\n", n[0], n[1], n[2]))
    for a, b, c in F.tolist():
        out.append("f %u//%u %u//%u %u//%u\n" % (c + 1, c + 1, b + 1, b + 1, a + 1, a + 1))
    return "".join(out)


def parse_ply(text):
    """(V, N, C uint8, F) of an ASCII PLY as nrs_mesh_write lays it out"""
    lines = text.split("\n")
    nv = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[-1])
    nf = int([ln for ln in lines if ln.startswith("element face")][0].split()[-1])
    body = lines[lines.index("end_header") + 1:]
    rows = np.array([[float(t) for t in ln.split()] for ln in body[:nv]], np.float64).reshape(nv, 9)
    faces = np.array([[int(t) for t in ln.split()[1:]] for ln in body[nv:nv + nf]], np.int64).reshape(nf, 3)
    return rows[:, :3], rows[:, 3:6], rows[:, 6:9].astype(np.uint8), faces


def all_masks():
    return itertools.product(range(2), repeat=8)
