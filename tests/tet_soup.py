"""Synthetic tet meshes whose cell -> tet look-up table is known BY CONSTRUCTION (numpy only: no GPU, no oracle).

The regular Kuhn lattices of synth.make_cage_edit reach only some of the device build's branches (nrs_cage.hip: lane teams by mesh size, the 128-cell hit mask,
the sort tiers by list length).  A "tet soup" reaches the others on purpose: its building block is a tiny tet -- four vertices within 1/16 of a cascade-0 cell
(1/128) of a point that lies at least 1/4 cell from every face of its cascade-0 cell.  The cell borders of cascade L are a subset of the cascade-0 face planes
(0.5 + (i / 128 - 0.5) 2^L is a multiple of 1/128), so such a tet lies strictly inside exactly ONE cell of each of the five cascades and contributes exactly one
entry per cascade, at level * 128^3 + morton(cell_of(centre, level)).  How many tets stand in a cell is then the recipe's choice: list lengths of exactly 24,
25, 128, 129 or 20 000 are a matter of counting.  Everything stays inside (0.05, 0.95)^3: no clamped border cell is involved.

tests/test_tet_soup_host.py holds this construction against the oracle's builder and the host builder; tests/test_gpu_cage_lut_shapes.py holds the device
build against it.
"""
import collections

import numpy as np

from nerfshop_amd import synth

GRID = 128
GRID_VOL = GRID ** 3
CASCADES = 5
N_CELLS = CASCADES * GRID_VOL
CELL = 1.0 / GRID
KSMALL, KMID, KLDS = 24, 128, 16384   # nrs_cage.hip: kSmallList, kMidList, kSortLdsEntries
BITMAP_MAX_TETS = 15360 * 32          # lut_sort_big_kernel: the bitmap pass while (n_tets + 31) / 32 <= kSortScanWords

# edit: synth.CageEdit; offsets [N_CELLS + 1] uint32, idx uint32 (ascending per cell), max_per_cell int: the expected table; centres [n_tets, 3] float64 (final tet order)
Soup = collections.namedtuple("Soup", "edit offsets idx max_per_cell centres")


def cell_of(p, level):
    """get_cell_at_pos (selection_utils.cu:70-83) in float32, operation by operation as the kernels' cell_of: [n, 3] positions -> [n, 3] int32 cells of cascade `level`."""
    p = np.asarray(p, np.float32)
    s = np.float32(2.0 ** -level)
    q = (p - np.float32(0.5)) * s + np.float32(0.5)
    return np.clip((q * np.float32(GRID)).astype(np.int32), 0, GRID - 1)


def cell_ids(p, level):
    """Index into the offsets array of the cascade-`level` cell of each position."""
    c = cell_of(p, level).astype(np.uint32)
    return np.uint32(level * GRID_VOL) + synth.morton3d(c[:, 0], c[:, 1], c[:, 2])


def csr_from_entries(cells, tets):
    """(cell, tet) pairs in any order -> (offsets [N_CELLS + 1] uint32, idx uint32 ascending inside each cell, longest list)."""
    cells, tets = np.asarray(cells, np.int64), np.asarray(tets, np.uint32)
    order = np.lexsort((tets, cells))
    counts = np.bincount(cells, minlength=N_CELLS)
    offsets = np.zeros(N_CELLS + 1, np.uint32)
    offsets[1:] = np.cumsum(counts)
    return offsets, np.ascontiguousarray(tets[order]), int(counts.max()) if counts.size else 0


def csr_entries(offsets, idx):
    """The inverse: a table's (cell, tet) pairs, cell-major."""
    return np.repeat(np.arange(N_CELLS, dtype=np.int64), np.diff(offsets.astype(np.int64))), np.asarray(idx, np.uint32)


def bitfield_of(offsets):
    """Touched-cell bitfield of a table: bit (c & 7) of byte (c >> 3) is set when cell c's list is not empty."""
    return np.packbits(np.diff(offsets.astype(np.int64)) > 0, bitorder="little")


def list_lengths(offsets, level=None):
    n = np.diff(offsets.astype(np.int64))
    return n if level is None else n[level * GRID_VOL:(level + 1) * GRID_VOL]


def centres_in_cells(cells, rng):
    """One admissible centre per given cascade-0 cell ([n, 3] ints): the cell's middle, moved by up to 0.2 cell per axis (the bar is 1/4)."""
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    return (cells + 0.5 + rng.uniform(-0.2, 0.2, size=cells.shape)) * CELL


def distinct_cells(n, rng, lo=10, hi=118):
    """n distinct cascade-0 cells with every coordinate in [lo, hi), in random order.  (0.05, 0.95)^3 holds the cells 7 .. 120 entirely; the default leaves
    three cells on each side for a soup that is translated later.)"""
    side = hi - lo
    assert 7 <= lo and hi <= 121 and n <= side ** 3
    flat = rng.permutation(side ** 3)[:n]
    return np.stack([flat // (side * side), (flat // side) % side, flat % side], 1).astype(np.int64) + lo


_DIRS = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64) / np.sqrt(3.0)


def _edit(vertices, tets):
    vertices = np.ascontiguousarray(vertices, np.float32)
    return synth.CageEdit(vertices=vertices, original_vertices=vertices.copy(), tets=np.ascontiguousarray(tets, np.uint32), local_rotations=None, copy=False)


def tiny_soup(centres, counts, seed):
    """counts[i] tiny tets round centres[i] (each with four vertices of its own, the tets in shuffled order so that no list arrives ascending) -> Soup."""
    centres = np.asarray(centres, np.float64).reshape(-1, 3)
    counts = np.asarray(counts, np.int64).reshape(-1)
    assert centres.shape[0] == counts.shape[0] and (counts >= 0).all()
    assert (centres > 0.05).all() and (centres < 0.95).all(), "soup geometry stays inside (0.05, 0.95)^3"
    frac = centres * GRID - np.floor(centres * GRID)
    assert (frac >= 0.25).all() and (frac <= 0.75).all(), "a centre lies at least 1/4 cell from every face of its cascade-0 cell"
    rng = np.random.default_rng(seed)
    n = int(counts.sum())
    order = rng.permutation(n)                       # final tet k is the order[k]-th tet of the cluster-major list
    c = np.repeat(centres, counts, axis=0)[order]
    # a regular tet of circumradius 0.45 .. 0.9 of the allowance (1/16 cell), its corners in one of the 24 orders and each moved by up to 0.05 of it
    radius = rng.uniform(0.45, 0.9, size=(n, 1, 1)) * (CELL / 16.0)
    corner = np.argsort(rng.random((n, 4)), axis=1)
    v = c[:, None, :] + radius * (_DIRS[corner] + rng.uniform(-0.05, 0.05, size=(n, 4, 3)))
    vertices = v.reshape(-1, 3).astype(np.float32)
    tets = np.arange(4 * n, dtype=np.uint32).reshape(n, 4)
    # the construction's premises, on the float32 vertices the builders see
    v32 = vertices.astype(np.float64).reshape(n, 4, 3)
    assert (np.linalg.norm(v32 - c[:, None, :], axis=2) <= CELL / 16.0).all()
    vol = np.abs(np.linalg.det(v32[:, 1:] - v32[:, :1])) / 6.0
    assert (vol > 1e-3 * (CELL / 16.0) ** 3).all(), "degenerate tet"
    cells, ids = [], np.arange(n, dtype=np.uint32)
    for level in range(CASCADES):
        cid = cell_ids(c, level)
        for k in range(4):
            assert np.array_equal(cell_ids(vertices[k::4], level), cid)
        cells.append(cid.astype(np.int64))
    offsets, idx, mx = csr_from_entries(np.concatenate(cells), np.tile(ids, CASCADES))
    return Soup(_edit(vertices, tets), offsets, idx, mx, c)


def big_tet_bounds(box):
    """A box in cascade-0 cells ((x0, y0, z0), (nx, ny, nz)) -> its corners in world units: from 0.3 cell inside the first cell to 0.3 cell before the end of
    the last, so that the float32 cell_of of the bounds is the box asked for."""
    (x0, y0, z0), (nx, ny, nz) = box
    lo = (np.array([x0, y0, z0], np.float64) + 0.3) * CELL
    hi = (np.array([x0 + nx, y0 + ny, z0 + nz], np.float64) - 0.3) * CELL
    return lo, hi


def with_big_tets(soup, boxes, at):
    """Append one large tet per box (the corner tet at the box's low corner: lo, lo + dx, lo + dy, lo + dz) and swap it to tet index at[i], so that it shares
    a wave with tiny ones.  The tables of large tets are not known by construction: returns (edit, tiny_cells, tiny_tets, big_ids) -- the tiny tets' expected
    (cell, tet) pairs under the new numbering and the large tets' indices; the caller adds the large tets' pairs from a builder it trusts and calls
    csr_from_entries."""
    e = soup.edit
    n_old, k = e.tets.shape[0], len(boxes)
    at = np.asarray(at, np.int64)
    assert at.shape[0] == k and len(set(at.tolist())) == k and (at >= 0).all() and (at < n_old + k).all()
    new_v, new_t = [], []
    for i, box in enumerate(boxes):
        lo, hi = big_tet_bounds(box)
        assert (lo > 0.05).all() and (hi < 0.95).all()
        new_v += [lo, [hi[0], lo[1], lo[2]], [lo[0], hi[1], lo[2]], [lo[0], lo[1], hi[2]]]
        base = e.vertices.shape[0] + 4 * i
        new_t.append([base, base + 1, base + 2, base + 3])
    vertices = np.concatenate([e.vertices, np.array(new_v, np.float32)])
    tets = np.concatenate([e.tets, np.array(new_t, np.uint32)])
    number = np.arange(n_old + k, dtype=np.int64)    # number[old index] = new index
    for i in range(k):                               # swap the rows n_old + i and at[i]
        a, b = n_old + i, int(at[i])
        tets[[a, b]] = tets[[b, a]]
        ia, ib = np.flatnonzero(number == a)[0], np.flatnonzero(number == b)[0]
        number[ia], number[ib] = b, a
    big_ids = number[n_old:].astype(np.uint32)
    cells, t = csr_entries(soup.offsets, soup.idx)
    return _edit(vertices, tets), cells, number[t].astype(np.uint32), big_ids


def translated(edit, cells_xyz):
    """The same soup moved by whole cascade-0 cells.  (x + k / 128 is not exact in float32, but a shift of the order of an ulp is nothing against the
    1/4 - 1/16 cell every vertex keeps from its cell's faces: the caller shifts the centres too and asks tiny_soup's expected cells for them.)"""
    return (edit.vertices.astype(np.float64) + np.asarray(cells_xyz, np.float64) * CELL).astype(np.float32)


def expected_for_centres(centres):
    """Expected table of tiny tets standing round `centres` (final tet order), as tiny_soup computes it."""
    n = centres.shape[0]
    cells = np.concatenate([cell_ids(centres, level).astype(np.int64) for level in range(CASCADES)])
    return csr_from_entries(cells, np.tile(np.arange(n, dtype=np.uint32), CASCADES))


# ---- recipes shared by the host test (against the oracle) and the GPU test (against the device build) ------------------------------------------------
BOUNDARY_LENGTHS = (1, 2, 23, 24, 25, 127, 128, 129, 1025)


def boundary_recipe(seed, pad_to=None):
    """Clusters of exactly 1, 2, 23, 24, 25, 127, 128, 129 and 1 025 tets in distinct cascade-0 cells, three cells of each (4 452 tets); pad_to: single tets in
    further cells up to that many tets.  -> (centres, counts)"""
    rng = np.random.default_rng(seed)
    counts = np.repeat(np.array(BOUNDARY_LENGTHS, np.int64), 3)
    n_single = 0 if pad_to is None else pad_to - int(counts.sum())
    assert n_single >= 0
    cells = distinct_cells(counts.size + n_single, rng)
    return centres_in_cells(cells, rng), np.concatenate([counts, np.ones(n_single, np.int64)])


BITONIC_N_TETS = 491537   # (n + 31) / 32 == 15361: one word more than the bitmap pass takes; neither a multiple of 8 nor of 64


def bitonic_recipe(seed, every=1):
    """The soup of the bitonic tiers: one cascade-0 cell of 20 000 tets (longer than kSortLdsEntries at every cascade: the network in HBM), one of 16 385 (the first length
    that leaves LDS) and cells of 16 384 .. 129 (the network in LDS), 128 .. 25 (a wave) and 24 .. 1 (a thread); BITONIC_N_TETS in all.  every = 16: the same
    cells and centres with a sixteenth (rounded up) of each cluster -- the recipe's geometry at a size a CPU builder answers quickly.  -> (centres, counts)"""
    rng = np.random.default_rng(seed)
    counts = [20000, 16385, 16384, 16384, 16383, 12000, 8000, 8000, 5000, 4097, 4096, 3000] + [2000] * 20 + [1025, 1024, 1023] + [600] * 60 + [300] * 100 + [130] * 60 + [129] * 60
    counts += [128] * 150 + [127] * 50 + [100] * 200 + [64, 65, 63] * 40 + [40] * 300 + [26] * 100 + [25] * 150
    counts += [24] * 300 + [23] * 100 + [12] * 1000 + [3] * 2000 + [2] * 3000
    counts = np.array(counts, np.int64)
    n_single = BITONIC_N_TETS - int(counts.sum())
    assert n_single > 0
    counts = np.concatenate([counts, np.ones(n_single, np.int64)])
    cells = distinct_cells(counts.size, rng)
    centres = centres_in_cells(cells, rng)
    if every > 1:
        counts = (counts + every - 1) // every
    return centres, counts
