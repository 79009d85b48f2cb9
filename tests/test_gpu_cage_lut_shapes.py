"""The device build of the cell -> tet look-up table (nrs_cage.hip: count -> scan -> fill -> per-cell sort) at the launch shapes and list lengths that the
regular lattices of tests/test_gpu_cage_update.py and tests/test_gpu_fine_lut.py never produce:

  a  a small mesh (<= 16 384 tets) of small tets: 8-lane teams at cascade 0 (tet_mark_kernel<FILL, 8> with `small`)
  b  boxes of more than 128 cells under 1-lane teams and under a large mesh's 8-lane teams (the lattices' large meshes stay below 91 and 13 cells; only the small
     aabb-16 cage goes beyond the mask, with 8 lanes): the fill pass's own cell_meets_tet beyond the hit mask, mask words filled over 16 and 128 trips, waves
     whose items differ widely in box size, last waves with dead items
  c  lists of exactly 1, 2, 23, 24, 25, 127, 128, 129 and 1 025 tets (kSmallList = 24, kMidList = 128), under both team layouts
  d  more than 491 520 tets: no bitmap pass, lut_sort_big_kernel's bitonic networks in LDS (129 .. 16 384 entries) and in HBM (more)
  e  in a to c a rebuild back to the first pose: every path of the fill pass leaves `counts` zeroed for the next build
  f  meshes of five and six tets: every segment shorter than one wave

Everything is integer: tables are compared with np.array_equal.  The expected tables are the oracle's (oracle.tet_lut_build) and, for tet soups, the
construction of tests/tet_soup.py, which tests/test_tet_soup_host.py holds against the oracle and the host builder.  Each test first asserts, on the CPU
from the mesh and the expected table, that the branch it is named after is reached: `_teams` and `_cells0` restate launch_tet_mark / build_lut_on_device.
"""
import numpy as np
import pytest

import tet_soup as ts

pytestmark = pytest.mark.gpu

SHIFT = (3, -2, 1)   # a move by whole cascade-0 cells: a soup's construction holds for the moved centres


def _cells0(verts, n_tets):
    """build_lut_on_device's estimate of the cascade-0 cells in a tet's box, from the bounding box of `verts` (the operator's box when the build starts)."""
    ext = np.maximum(verts.max(0).astype(np.float32) - verts.min(0).astype(np.float32), np.float32(0)).astype(np.float64)
    side = np.cbrt(ext.prod() / max(n_tets / 6.0, 1.0)) * 128
    return float(np.float32((side + 1.0) ** 3))


def _teams(n_tets, cells0):
    """launch_tet_mark: lanes per (tet, cascade) item at each of the five cascades."""
    if n_tets <= 16384:
        return (64 if cells0 >= 32.0 else 8, 8, 8, 8, 8)
    return (8, 8, 1, 1, 1)


def _box_cells(verts, tets, level):
    """Cells of cascade `level` in each tet's bounding box, from the float32 cell_of of its bounds."""
    v = verts[tets]
    return (ts.cell_of(v.max(1), level) - ts.cell_of(v.min(1), level) + 1).astype(np.int64).prod(1)


def _explain(got_off, got_idx, off, idx):
    """Where two tables differ: the first cells, with cascade, length and the two lists' heads (a failure must be diagnosable from its message)."""
    if got_idx.size != idx.size and np.array_equal(got_off, off):
        return f"{got_idx.size} entries downloaded, {idx.size} expected, the offsets agree"
    if not np.array_equal(got_off, off):
        bad = np.flatnonzero(np.diff(got_off.astype(np.int64)) != np.diff(off.astype(np.int64)))
        return f"{bad.size} cells differ in length, first {[(int(c) // ts.GRID_VOL, int(c) % ts.GRID_VOL, int(got_off[c + 1]) - int(got_off[c]), int(off[c + 1]) - int(off[c])) for c in bad[:8]]} (cascade, morton, got, expected)"
    pos = np.flatnonzero(got_idx != idx)
    cells = np.unique(np.searchsorted(off, pos, side="right") - 1)
    out = [f"{pos.size} entries in {cells.size} cells differ"]
    for c in cells[:6]:
        a, b = got_idx[off[c]:off[c + 1]], idx[off[c]:off[c + 1]]
        first = int(np.flatnonzero(a != b)[0])
        out.append(f"cascade {int(c) // ts.GRID_VOL} cell {int(c) % ts.GRID_VOL} n={a.size} sorted={bool((np.diff(a.astype(np.int64)) > 0).all())} same-set={np.array_equal(np.sort(a), b)} "
                   f"first at {first}: got {a[first:first + 4].tolist()} expected {b[first:first + 4].tolist()}")
    return "; ".join(out)


def _check(op, expected, orig_bits=None):
    off, idx, mx = expected
    got = op.download(rotations=False)
    same = got["lut_idx"].size == idx.size and np.array_equal(got["lut_offsets"], off) and np.array_equal(got["lut_idx"], idx)
    assert same, _explain(got["lut_offsets"], got["lut_idx"], off, idx)
    assert op.lut_size() == (idx.size, mx)
    if orig_bits is not None:
        assert np.array_equal(got["original_bitfield"], orig_bits)


def _oracle_table(orc, verts, tets):
    off, idx, _, mx = orc.tet_lut_build(verts, tets)
    return off, idx, mx


def _create_move_and_back(rig, edit, first, moved_verts, moved):
    """One create and two rebuilds: the tables after creation, after a move, and after the move back (e: `counts` was left zeroed by whatever paths ran)."""
    op = rig.rt.CageDeformation(rig.ctx, rig.scene.desc, edit, device_authoring=True)
    try:
        _check(op, first, ts.bitfield_of(first[0]))   # (vertices == original_vertices in every mesh here but a's, which passes its own)
        op.update_vertices(None, moved_verts)
        _check(op, moved)
        op.update_vertices(None, edit.vertices)
        _check(op, first)
    finally:
        op.close()


# ---- a ------------------------------------------------------------------------------------------------------------------------------------------------
def test_small_mesh_with_eight_lane_teams(rig):
    """The 6 000-tet lattice in a box of half the default size per axis: cells0 is about 15, below the 32 that give a wave per item."""
    synth, orc = rig.scene.synth, rig.scene.orc
    mn, mx = np.array((0.22, 0.60, 0.40)), np.array((0.60, 0.76, 0.60))
    ctr, half = 0.5 * (mn + mx), 0.25 * (mx - mn)
    e = synth.make_cage_edit(lattice_n=10, box=(tuple(ctr - half), tuple(ctr + half)), translate=(0.05, 0.025, 0.0))   # (half the default move, too)
    pose = orc.mvc_apply(e.mvc_weights, synth.deform_cage(e.cage_vertices, (0.025, -0.02, 0.015), 47.0))
    n = e.tets.shape[0]
    assert n == 6000
    # a build starts from the box of the pose before it: creation from e.vertices' (both of its builds), the move from e.vertices', the move back from the pose's
    for verts in (e.vertices, pose):
        c0 = _cells0(verts, n)
        print(f"cells0 = {c0:.1f}")
        assert c0 < 32.0 and _teams(n, c0) == (8, 8, 8, 8, 8)
    for verts in (e.original_vertices, e.vertices, pose):
        box0 = _box_cells(verts, e.tets, 0)
        assert (box0 > 8).any() and box0.max() <= 128   # more than one trip of an 8-lane team; the mask covers every box
    first, moved = _oracle_table(orc, e.vertices, e.tets), _oracle_table(orc, pose, e.tets)
    assert not np.array_equal(first[0], moved[0])
    orig_bits = ts.bitfield_of(_oracle_table(orc, e.original_vertices, e.tets)[0])
    assert np.array_equal(orig_bits, e.original_bitfield)
    op = rig.rt.CageDeformation(rig.ctx, rig.scene.desc, e, device_authoring=True)
    try:
        _check(op, first, orig_bits)
        op.update_vertices(None, pose)
        _check(op, moved)
        op.update_vertices(None, e.vertices)
        _check(op, first)
    finally:
        op.close()


# ---- b ------------------------------------------------------------------------------------------------------------------------------------------------
BIG_BOXES = [((20, 30, 40), (9, 9, 9)), ((14, 14, 14), (100, 100, 100)), ((40, 70, 80), (9, 9, 9)), ((30, 50, 20), (30, 12, 7)), ((60, 20, 30), (30, 12, 7))]


def test_boxes_beyond_the_hit_mask(rig):
    """A large mesh (8 lanes at cascades 0 and 1, one lane at 2 to 4) of 16 998 tiny tets and five large ones at the tet indices 3, 4, 8 191, 12 001 and
    n - 1: boxes of 729 and 2 520 cells at cascade 0 and of more than 128 at cascade 1 under 8-lane teams, a box of 100^3 cascade-0 cells that still holds
    more than 128 cells at cascades 2, 3 and 4 under 1-lane teams -- each in a wave whose other items have one cell."""
    orc = rig.scene.orc
    soup = ts.tiny_soup(*ts.boundary_recipe(5, pad_to=16998), seed=7)
    n = soup.edit.tets.shape[0] + len(BIG_BOXES)
    at = [3, 4, 8191, 12001, n - 1]
    edit, tiny_cells, tiny_tets, big = ts.with_big_tets(soup, BIG_BOXES, at)
    assert edit.tets.shape[0] == n == 17003 and n % 8 != 0 and n % 64 != 0 and big.tolist() == at
    assert _teams(n, _cells0(edit.vertices, n)) == (8, 8, 1, 1, 1)
    # dead items: the 8-lane segment [0, 2 n) and the 1-lane segment [2 n, 5 n) both end inside a wave, the latter with ONE live item
    assert (2 * n) % 8 == 6 and (3 * n) % 64 == 1
    moved_verts = ts.translated(edit, SHIFT)
    is_big = np.zeros(n, bool)
    is_big[big] = True
    for verts in (edit.vertices, moved_verts):
        box = np.stack([_box_cells(verts, edit.tets, level) for level in range(ts.CASCADES)])   # [5, n]
        assert (box[:, ~is_big] == 1).all()
        if verts is edit.vertices:
            for i, (lo_cell, size) in enumerate(BIG_BOXES):   # the boxes asked for, from the float32 cell_of of the bounds
                v = verts[edit.tets[big[i]]]
                lo, hi = ts.cell_of(v.min(0)[None], 0)[0], ts.cell_of(v.max(0)[None], 0)[0]
                assert lo.tolist() == list(lo_cell) and (hi - lo + 1).tolist() == list(size)
            assert box[0, big].tolist() == [729, 1000000, 729, 2520, 2520]
        print("cells per cascade in the large tets' boxes:", box[:, big].tolist())
        assert (box[0, big] > 128).all()                        # T = 8, cascade 0: beyond the mask; the mask words filled over all 16 trips
        assert (box[1, big[[1, 3, 4]]] > 128).all()             # T = 8, cascade 1 (the last of them is the segment's last item, in a wave with two dead teams)
        assert (box[2:, big[1]] > 128).all()                    # T = 1, cascades 2 to 4: beyond the mask; the mask words filled over all 128 trips
        assert ((box[2:, big[[0, 2, 3, 4]]] > 1) & (box[2:, big[[0, 2, 3, 4]]] < 128)).any()   # partial masks too
    # a wave holds 8 or 64 consecutive items -- tets consecutive modulo n -- and only five tets are large: every wave with a large tet has tiny ones beside it
    # (tets 3 and 4 share the first wave of cascade 0 with six tiny ones), so its trip count is set by __any over very different boxes
    assert len(big) < 8 and not is_big[:8].all()
    # expected: the oracle on the whole mesh -- and the same table from the construction of the tiny tets merged with the oracle's lists of the five large ones
    first = _oracle_table(orc, edit.vertices, edit.tets)
    off, idx, _, _ = orc.tet_lut_build(edit.vertices, edit.tets[big])
    big_cells, local = ts.csr_entries(off, idx)
    merged = ts.csr_from_entries(np.concatenate([tiny_cells, big_cells]), np.concatenate([tiny_tets, big[local]]))
    assert np.array_equal(merged[0], first[0]) and np.array_equal(merged[1], first[1]) and merged[2] == first[2]
    moved = _oracle_table(orc, moved_verts, edit.tets)
    assert not np.array_equal(first[0], moved[0])
    _create_move_and_back(rig, edit, first, moved_verts, moved)


# ---- c ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad_to", [None, 17001])
def test_list_length_boundaries(rig, pad_to):
    """Three cascade-0 cells each of exactly 1, 2, 23, 24, 25, 127, 128, 129 and 1 025 tets: the thread's insertion sort up to 24, the wave's network up to 128, the
    workgroup's bitmap pass beyond -- in a small mesh (a wave per item at cascade 0, 8 lanes elsewhere) and, padded with single tets, in a large one."""
    orc = rig.scene.orc
    soup = ts.tiny_soup(*ts.boundary_recipe(5, pad_to), seed=7)
    edit = soup.edit
    n = edit.tets.shape[0]
    assert n == (pad_to or 4452) and n <= ts.BITMAP_MAX_TETS
    assert _teams(n, _cells0(edit.vertices, n)) == ((64, 8, 8, 8, 8) if pad_to is None else (8, 8, 1, 1, 1))
    moved_verts = ts.translated(edit, SHIFT)
    assert _teams(n, _cells0(moved_verts, n)) == _teams(n, _cells0(edit.vertices, n))
    first = soup[1:4]
    moved = ts.expected_for_centres(soup.centres + np.array(SHIFT) * ts.CELL)
    for table in (first, moved):
        lengths = ts.list_lengths(table[0], 0)
        for length in ts.BOUNDARY_LENGTHS:
            assert (lengths == length).sum() >= 3, length
        every = ts.list_lengths(table[0])
        n_long, n_mid = int((every > ts.KMID).sum()), int(((every > ts.KSMALL) & (every <= ts.KMID)).sum())
        assert n_long >= 3 and n_mid >= 9   # both ends of the big_cells worklist are in use
    assert not np.array_equal(first[0], moved[0])
    if pad_to is None:   # the construction once more against the oracle, at the very mesh (0.1 s)
        o = _oracle_table(orc, edit.vertices, edit.tets)
        assert np.array_equal(o[0], first[0]) and np.array_equal(o[1], first[1]) and o[2] == first[2]
    _create_move_and_back(rig, edit, first, moved_verts, moved)


# ---- d ------------------------------------------------------------------------------------------------------------------------------------------------
def test_bitonic_tiers(rig):
    """491 537 tets, one word of bitmap more than the bitmap pass takes: every list of more than 128 tets is sorted by a bitonic network -- in LDS up to
    16 384 entries, in HBM beyond (a cascade-0 cell of 20 000 tets and one of 16 385, and the coarser cells that hold them).  Built at creation, then rebuilt
    with the whole soup moved by (3, -2, 1) cells: the rebuild also finds `counts` as these paths left it."""
    orc = rig.scene.orc
    centres, counts = ts.bitonic_recipe(11)
    soup = ts.tiny_soup(centres, counts, seed=13)
    edit = soup.edit
    n = edit.tets.shape[0]
    assert n == ts.BITONIC_N_TETS and (n + 31) // 32 == 15361 and n > ts.BITMAP_MAX_TETS   # (n + 31) / 32 <= kSortScanWords = 15 360 fails: no bitmap pass
    assert _teams(n, _cells0(edit.vertices, n)) == (8, 8, 1, 1, 1)
    moved_verts = ts.translated(edit, SHIFT)
    first = soup[1:4]
    moved = ts.expected_for_centres(soup.centres + np.array(SHIFT) * ts.CELL)
    assert not np.array_equal(first[0], moved[0])
    for table in (first, moved):
        for level in range(ts.CASCADES):
            lengths = ts.list_lengths(table[0], level)
            hbm, lds = int((lengths > ts.KLDS).sum()), int(((lengths > ts.KMID) & (lengths <= ts.KLDS)).sum())
            mid, small = int(((lengths > ts.KSMALL) & (lengths <= ts.KMID)).sum()), int(((lengths > 0) & (lengths <= ts.KSMALL)).sum())
            if table is first:
                print(f"cascade {level}: {hbm} lists in HBM, {lds} in LDS, {mid} by a wave, {small} by a thread; longest {int(lengths.max())}")
            assert hbm >= 1 and lds >= 300   # both networks at every cascade
        every = ts.list_lengths(table[0])
        assert int(((every > ts.KSMALL) & (every <= ts.KMID)).sum()) >= 1000 and int(((every > 1) & (every <= ts.KSMALL)).sum()) >= 1000   # a wave's, a thread's
        lengths0 = ts.list_lengths(table[0], 0)
        for length in (24, 25, 128, 129, 16384, 16385, 20000):
            assert (lengths0 == length).any(), length
        assert table[2] > 20000   # (every cascade's longest list exceeds kFineMaxList: no fine table is built)
    # the recipe's geometry at this scale against the oracle: the same cells and centres with a sixteenth of each cluster
    c16, n16 = ts.bitonic_recipe(11, every=16)
    assert np.array_equal(c16, centres)
    s16 = ts.tiny_soup(c16, n16, seed=13)
    o = _oracle_table(orc, s16.edit.vertices, s16.edit.tets)
    assert np.array_equal(o[0], s16.offsets) and np.array_equal(o[1], s16.idx) and o[2] == s16.max_per_cell
    op = rig.rt.CageDeformation(rig.ctx, rig.scene.desc, edit, device_authoring=True)
    try:
        _check(op, first, ts.bitfield_of(first[0]))
        op.update_vertices(None, moved_verts)
        _check(op, moved)
    finally:
        op.close()


# ---- f ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_big", [False, True])
def test_segments_shorter_than_a_wave(rig, with_big):
    """Five tiny tets in two cells (8-lane teams, five items per segment: less than the eight of one wave) and the same with a 9 x 9 x 9-cell tet (a wave per
    item at cascade 0: six waves in two workgroups, the second half empty)."""
    orc = rig.scene.orc
    rng = np.random.default_rng(4)
    cells = np.array([[40, 41, 42], [41, 41, 42]])
    soup = ts.tiny_soup(ts.centres_in_cells(cells, rng), [3, 2], seed=5)
    edit = soup.edit
    if with_big:
        edit, _, _, big = ts.with_big_tets(soup, [((36, 37, 38), (9, 9, 9))], at=[2])
        assert big.tolist() == [2]
    n = edit.tets.shape[0]
    moved_verts = ts.translated(edit, SHIFT)
    for verts in (edit.vertices, moved_verts):
        assert _teams(n, _cells0(verts, n)) == ((64, 8, 8, 8, 8) if with_big else (8, 8, 8, 8, 8))
    first, moved = _oracle_table(orc, edit.vertices, edit.tets), _oracle_table(orc, moved_verts, edit.tets)
    if not with_big:
        assert np.array_equal(first[0], soup.offsets) and np.array_equal(first[1], soup.idx)
    else:
        assert _box_cells(edit.vertices, edit.tets, 0).tolist() == [1, 1, 729, 1, 1, 1]
    _create_move_and_back(rig, edit, first, moved_verts, moved)
