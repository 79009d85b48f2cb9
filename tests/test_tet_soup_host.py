"""tests/tet_soup.py builds meshes whose cell -> tet table is known by construction; tests/test_gpu_cage_lut_shapes.py holds the device build against that
construction.  Here the construction itself is held against the project's two CPU builders -- the oracle's (oracle/nrs_oracle.cpp build_tet_lut) and the host
builder of nrs_authoring.cpp (synth.build_tet_lut) -- so that the GPU tests do not rest on an unchecked reference.  No GPU.

Oracle wall time (measured, 16 CPU threads): 0.19 s for the 20 000-tet soup below (the host builder: 2.1 s), 0.52 s for the sixteenth of the bitonic recipe
(159 900 tets), 0.44 s for the 17 003-tet soup with five large tets (291 394 entries).  Extrapolated to the 491 537 tets of the full bitonic recipe: about
5 s -- affordable once, too long for a test that runs with every suite; the GPU test asks the oracle for the sixteenth."""
import time

import numpy as np
import pytest

import tet_soup as ts


@pytest.fixture(scope="module")
def builders(built):
    from nerfshop_amd import synth
    from oracle import oracle as orc
    return orc.tet_lut_build, synth.build_tet_lut


def _same(table, soup_table):
    off, idx, bits, mx = table
    e_off, e_idx, e_mx = soup_table
    assert np.array_equal(off, e_off)
    assert np.array_equal(idx, e_idx)
    assert mx == e_mx
    assert np.array_equal(bits, ts.bitfield_of(e_off))


def test_cell_of_and_csr_helpers():
    # cell borders of every cascade are cascade-0 face planes: the centre of cascade-0 cell (x, y, z) lies in the cascade-L cell ((x - 64) >> L) + 64 per axis
    rng = np.random.default_rng(1)
    cells = ts.distinct_cells(4096, rng)
    p = ts.centres_in_cells(cells, rng)
    for level in range(ts.CASCADES):
        assert np.array_equal(ts.cell_of(p, level), ((cells - 64) >> level) + 64)
    off, idx, mx = ts.csr_from_entries([5, 3, 5, 5, ts.N_CELLS - 1], [9, 1, 2, 7, 4])
    assert mx == 3 and off[3] == 0 and off[4] == 1 and off[5] == 1 and off[6] == 4 and off[-1] == 5
    assert idx.tolist() == [1, 2, 7, 9, 4]
    c, t = ts.csr_entries(off, idx)
    assert c.tolist() == [3, 5, 5, 5, ts.N_CELLS - 1] and t.tolist() == idx.tolist()
    bits = ts.bitfield_of(off)
    assert bits.size == ts.N_CELLS // 8 and bits[0] == (1 << 3) | (1 << 5) and bits[-1] == 1 << 7 and int(np.unpackbits(bits).sum()) == 3


def test_random_soup_2000(builders):
    """2 000 tets in clusters of random size; lists arrive unsorted (the tet order is shuffled)."""
    oracle_build, host_build = builders
    rng = np.random.default_rng(2)
    counts = 1 + rng.multinomial(1900, rng.dirichlet(np.ones(100)))
    soup = ts.tiny_soup(ts.centres_in_cells(ts.distinct_cells(100, rng), rng), counts, seed=3)
    assert soup.edit.tets.shape[0] == 2000
    cells0 = ts.cell_ids(soup.centres, 0)
    assert (np.diff(cells0.astype(np.int64)) < 0).any()   # really shuffled
    _same(oracle_build(soup.edit.vertices, soup.edit.tets), soup[1:4])
    _same(host_build(soup.edit.vertices, soup.edit.tets), soup[1:4])


@pytest.mark.parametrize("pad_to", [None, 20000])
def test_boundary_soups(builders, pad_to):
    """Clusters of exactly 1, 2, 23, 24, 25, 127, 128, 129 and 1 025 tets (4 452 tets), alone and padded to 20 000 tets with singles."""
    oracle_build, host_build = builders
    soup = ts.tiny_soup(*ts.boundary_recipe(5, pad_to), seed=7)
    assert soup.edit.tets.shape[0] == (pad_to or 4452)
    lengths = ts.list_lengths(soup.offsets, 0)
    for n in ts.BOUNDARY_LENGTHS:
        assert (lengths == n).sum() >= 3
    t0 = time.perf_counter()
    table = oracle_build(soup.edit.vertices, soup.edit.tets)
    print(f"oracle, {soup.edit.tets.shape[0]} tets: {time.perf_counter() - t0:.2f} s")
    _same(table, soup[1:4])
    _same(host_build(soup.edit.vertices, soup.edit.tets), soup[1:4])


def test_translated_soup(builders):
    """A soup moved by whole cells keeps its construction: the expected cells are those of the moved centres."""
    oracle_build, _ = builders
    soup = ts.tiny_soup(*ts.boundary_recipe(5), seed=7)
    shift = (3, -2, 1)
    verts = ts.translated(soup.edit, shift)
    expected = ts.expected_for_centres(soup.centres + np.array(shift) * ts.CELL)
    assert not np.array_equal(expected[0], soup.offsets)
    _same(oracle_build(verts, soup.edit.tets), expected)


def test_bitonic_recipe_at_a_sixteenth(builders):
    """The recipe of the bitonic tiers: its populations at full size (from the construction alone), its geometry against the oracle at a sixteenth of each cluster."""
    oracle_build, _ = builders
    centres, counts = ts.bitonic_recipe(11)
    assert int(counts.sum()) == ts.BITONIC_N_TETS and (ts.BITONIC_N_TETS + 31) // 32 == 15361
    assert int((counts > ts.KLDS).sum()) == 2 and int(counts.max()) == 20000
    c16, n16 = ts.bitonic_recipe(11, every=16)
    assert np.array_equal(c16, centres) and np.array_equal(n16, (counts + 15) // 16)
    soup = ts.tiny_soup(c16, n16, seed=13)
    _same(oracle_build(soup.edit.vertices, soup.edit.tets), soup[1:4])


def test_big_tets_merge(builders):
    """with_big_tets: the oracle's lists of the large tets alone, merged per cell with the constructed lists of the tiny ones, are the oracle's table of the whole mesh."""
    oracle_build, _ = builders
    soup = ts.tiny_soup(*ts.boundary_recipe(5), seed=7)
    boxes = [((20, 30, 40), (9, 9, 9)), ((60, 20, 30), (30, 12, 7)), ((12, 14, 16), (40, 40, 40))]
    n = soup.edit.tets.shape[0] + len(boxes)
    edit, tiny_cells, tiny_tets, big = ts.with_big_tets(soup, boxes, at=[3, 2000, n - 1])
    assert big.tolist() == [3, 2000, n - 1] and edit.tets.shape[0] == n
    for i, (lo_cell, size) in enumerate(boxes):   # the float32 bounds of each large tet span the box asked for
        v = edit.vertices[edit.tets[big[i]]]
        lo, hi = ts.cell_of(v.min(0)[None], 0)[0], ts.cell_of(v.max(0)[None], 0)[0]
        assert lo.tolist() == list(lo_cell) and (hi - lo + 1).tolist() == list(size)
    off, idx, _, _ = oracle_build(edit.vertices, edit.tets[big])
    big_cells, local = ts.csr_entries(off, idx)
    expected = ts.csr_from_entries(np.concatenate([tiny_cells, big_cells]), np.concatenate([tiny_tets, big[local]]))
    _same(oracle_build(edit.vertices, edit.tets), expected)
