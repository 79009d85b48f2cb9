"""The selection tool's host side (include/nrs.h "selection tool"): nrs_selection_reset / _grow / _upscale and the accessors against the deque restatement of
tests/selection_ref.py -- the cell list L with its order and duplicates, the bitfield S, the queue's length and the level -- and nrs_bitfield_morph_host against the numpy
shift-and-combine reference.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import selection_ref as ref

VOL, G = ref.VOL, ref.G


def cell(x, y, z, level=0):
    return level * VOL + int(ref.morton(x, y, z))


@pytest.fixture(scope="module")
def grid(built):
    """seeded random densities below the thresholds used here, with a dense blob at every level: a ball in the interior, and a box that reaches the x = 0 face"""
    rng = np.random.default_rng(128)
    g = rng.uniform(0.0, 0.009, ref.CASCADES * VOL).astype(np.float32)
    a = np.arange(G)
    ball = (a[:, None, None] - 60) ** 2 + (a[None, :, None] - 64) ** 2 + (a[None, None, :] - 70) ** 2 <= 9 ** 2
    box = np.zeros((G, G, G), bool)
    box[0:4, 30:34, 30:34] = True
    dense = ref.morton_of_grid()[ball | box]
    for level in range(ref.CASCADES):
        g[level * VOL + dense] = rng.uniform(0.02, 5.0, dense.size).astype(np.float32)
    g.setflags(write=False)
    return g


def pair(grid, max_cascade=0):
    from nerfshop_amd import runtime as rt
    return rt.GrowingSelection(None, grid, max_cascade), ref.Growing(grid, max_cascade)


def assert_same(sel, model):
    assert np.array_equal(sel.selection_cell_idx, np.array(model.cells, np.uint32))          # order and duplicates
    assert np.array_equal(sel.selection_grid_bitfield, model.bitfield())
    assert sel.queue_size == len(model.queue) and sel.growing_level == model.level
    pts = sel.selection_points
    assert np.array_equal(pts.view(np.uint32), ref.cell_pos(model.cells).reshape(-1, 3).view(np.uint32))


def test_seeds_are_lifted_or_dropped_and_enter_the_list_only(grid):
    sel, model = pair(grid)
    seeds = [cell(60, 64, 70, 0), cell(40, 41, 42, 1), cell(64, 64, 64, 2), cell(3, 5, 7, 0), cell(64, 64, 64, 3)]
    for s in (sel.reset_growing, model.reset):
        s(seeds, 1)
    assert_same(sel, model)
    L = sel.selection_cell_idx
    assert len(L) == 3 and (L // VOL == 1).all()                      # the two seeds above level 1 are gone
    assert L[0] == ref.upper_cell(seeds[0], 1) and L[1] == seeds[1] and L[2] == ref.upper_cell(seeds[3], 1)
    assert not sel.selection_grid_bitfield.any() and sel.queue_size == 3 and not sel.performed_closing


@pytest.mark.parametrize("steps", [1, 7, 10000])
def test_budget(grid, steps):
    sel, model = pair(grid)
    seed = [cell(60, 64, 70)]
    sel.reset_growing(seed, 0)
    model.reset(seed, 0)
    popped = sel.grow_region(0.01, 0, steps)
    assert popped == model.grow(0.01, 0, steps)
    assert popped == steps or (1 < popped < steps and sel.queue_size == 0)   # min(steps, what the queue holds before it runs dry)
    assert_same(sel, model)


def test_two_calls_of_five_equal_one_of_ten(grid):
    a, _ = pair(grid)
    b, model = pair(grid)
    seed = [cell(60, 64, 70)]
    for s in (a, b):
        s.reset_growing(seed, 0)
    model.reset(seed, 0)
    assert a.grow_region(0.01, 0, 5) == 5 and a.grow_region(0.01, 0, 5) == 5 and b.grow_region(0.01, 0, 10) == 10
    model.grow(0.01, 0, 10)
    assert_same(a, model)
    assert_same(b, model)


def test_a_density_equal_to_the_threshold_is_accepted(grid):
    sel, model = pair(grid)
    seed = cell(60, 64, 70)
    threshold = float(grid[seed])
    sel.reset_growing([seed], 0)
    model.reset([seed], 0)
    assert sel.grow_region(threshold, 0, 1) == 1 and model.grow(threshold, 0, 1) == 1
    assert_same(sel, model)
    assert list(sel.selection_cell_idx) == [seed, seed] and sel.queue_size == 6
    sel.reset_growing([seed], 0)
    assert sel.grow_region(float(np.nextafter(np.float32(threshold), np.float32(np.inf))), 0, 1) == 1
    assert list(sel.selection_cell_idx) == [seed] and sel.queue_size == 0 and not sel.selection_grid_bitfield.any()


def test_an_empty_queue_is_a_no_op(grid):
    sel, model = pair(grid)
    sel.reset_growing([], 2)
    model.reset([], 2)
    assert sel.grow_region(0.01, 0, 100) == 0 and model.grow(0.01, 0, 100) == 0
    assert_same(sel, model)
    assert sel.growing_level == 2          # not even the level moves


def test_the_same_seed_twice(grid):
    sel, model = pair(grid)
    seed = cell(60, 64, 70)
    sel.reset_growing([seed, seed], 0)
    model.reset([seed, seed], 0)
    assert sel.grow_region(0.01, 0, 2) == 2 and model.grow(0.01, 0, 2) == 2
    assert_same(sel, model)
    assert list(sel.selection_cell_idx) == [seed, seed, seed]     # two seeds and one acceptance
    assert int(np.unpackbits(sel.selection_grid_bitfield).sum()) == 1


def test_a_grow_at_another_level_accepts_nothing(grid):
    sel, model = pair(grid, max_cascade=4)
    seeds = [cell(60, 64, 70), cell(61, 64, 70)]
    sel.reset_growing(seeds, 0)
    model.reset(seeds, 0)
    assert sel.grow_region(0.01, 1, 10000) == 2 and model.grow(0.01, 1, 10000) == 2
    assert_same(sel, model)
    assert sel.growing_level == 1 and len(sel.selection_cell_idx) == 2 and sel.queue_size == 0 and not sel.selection_grid_bitfield.any()


def test_a_boundary_cell_upscales_the_selection(grid):
    sel, model = pair(grid, max_cascade=2)
    seed = [cell(2, 31, 31)]                 # inside the box that reaches x = 0
    sel.reset_growing(seed, 0)
    model.reset(seed, 0)
    # grow one pop at a time up to the pop that accepts a cell of the x = 0 face
    while model.level == 0:
        n_before, q_before = len(model.cells), list(model.queue)
        assert sel.grow_region(0.01, model.level, 1) == 1 and model.grow(0.01, 0, 1) == 1
        assert_same(sel, model)
    trigger = q_before[0]
    assert ref.is_boundary(trigger % VOL) and sel.growing_level == 1
    L = sel.selection_cell_idx
    assert len(L) == n_before + 1 and (L // VOL == 1).all()                                    # the list keeps its length: nothing merged, the trigger appended
    assert L[-1] == ref.upper_cell(trigger, 1)
    flat = np.zeros(ref.CASCADES * VOL, np.uint8)
    flat[L] = 1
    assert np.array_equal(sel.selection_grid_bitfield, np.packbits(flat, bitorder="little"))   # S is exactly the bits of the lifted list
    lifted = [ref.upper_cell(q, 1) for q in q_before[1:]]
    assert list(model.queue)[:len(lifted)] == lifted                                          # the queue was lifted in place, the trigger's neighbours follow it
    # more growth at the new level agrees too, and a second upscale by hand
    assert sel.grow_region(0.01, 1, 300) == model.grow(0.01, 1, 300)
    assert_same(sel, model)
    sel.upscale_growing()
    model.upscale()
    assert_same(sel, model)
    assert sel.growing_level == 2
    sel.upscale_growing()                    # at max_cascade: nothing
    assert_same(sel, model)


def test_the_trigger_is_accepted_without_a_second_test(built):
    """a grid whose only dense cell lies on the x = 0 face: lifted to level 1 it lands on a cell of density 0, and is accepted all the same"""
    g = np.zeros(ref.CASCADES * VOL, np.float32)
    seed = cell(0, 50, 50)
    g[seed] = 1.0
    sel, model = pair(g, max_cascade=2)
    sel.reset_growing([seed], 0)
    model.reset([seed], 0)
    assert sel.grow_region(0.5, 0, 1) == 1 and model.grow(0.5, 0, 1) == 1
    assert_same(sel, model)
    up = ref.upper_cell(seed, 1)
    assert g[up] == 0.0 and list(sel.selection_cell_idx) == [up, up] and sel.growing_level == 1 and sel.queue_size == 6


def test_no_upscale_at_max_cascade(grid):
    sel, model = pair(grid, max_cascade=0)
    seed = [cell(0, 31, 31)]
    sel.reset_growing(seed, 0)
    model.reset(seed, 0)
    assert sel.grow_region(0.01, 0, 50) == model.grow(0.01, 0, 50)
    assert_same(sel, model)
    assert sel.growing_level == 0 and seed[0] in sel.selection_cell_idx[1:]        # the boundary cell is simply accepted
    assert sel.queue_size > 0


MORPH_CASES = [(op, se, r) for op in (ref.DILATE, ref.ERODE) for se in (ref.CUBE, ref.SPHERE) for r in (1, 2, 3)]


@pytest.mark.parametrize("name", ref.PATTERNS + ("random_inverse",))
def test_morph_host_against_numpy(built, name):
    from nerfshop_amd import runtime as rt
    level = ref.PATTERNS.index(name) % ref.CASCADES if name in ref.PATTERNS else 4
    bits = ref.grid_to_bits(ref.pattern(name), level)
    bits[(level + 1) % 5 * VOL // 8 + 17] = 0xA5       # another level of the input holds bits: not read, and zero in the output
    for op, se, r in MORPH_CASES:
        got = rt.bitfield_morph_host(bits, level, op, se, r)
        assert np.array_equal(got, ref.grid_to_bits(ref.pattern_morph(name, op, se, r), level)), (name, op, se, r)


def test_numpy_reference_against_the_tap_loop():
    """the reference itself, cell by cell against the loops of CubeSE / SphereSE, at radius 3 near set cells and near the faces"""
    rng = np.random.default_rng(5)
    for name in ("random", "corners", "slab_y"):
        g = ref.pattern(name)
        probes = np.concatenate([rng.integers(0, G, (40, 3)), rng.integers(0, 4, (20, 3)), G - 1 - rng.integers(0, 4, (20, 3))])
        for op, se in ((ref.DILATE, ref.SPHERE), (ref.ERODE, ref.CUBE), (ref.ERODE, ref.SPHERE)):
            want = ref.pattern_morph(name, op, se, 3)
            for x, y, z in probes:
                assert want[x, y, z] == ref.brute_cell(g, x, y, z, op, se, 3), (name, op, se, x, y, z)


def test_invalid_arguments_name_the_argument(built, grid):
    from nerfshop_amd import _abi
    lib = _abi.load()

    def refused(status, word):
        assert status == -1   # NRS_ERR_INVALID_ARG
        msg = lib.nrs_last_error().decode()
        assert word in msg, msg

    h = C.c_void_p()
    refused(lib.nrs_selection_create(grid.ctypes.data, grid.size - 1, 0, C.byref(h)), "n_floats")
    refused(lib.nrs_selection_create(grid.ctypes.data, grid.size, 5, C.byref(h)), "max_cascade")
    refused(lib.nrs_selection_create(None, grid.size, 0, C.byref(h)), "h_density_grid")
    assert lib.nrs_selection_create(grid.ctypes.data, grid.size, 4, C.byref(h)) == 0
    try:
        n = C.c_uint32()
        for bad in (float("nan"), float("inf"), float("-inf")):
            refused(lib.nrs_selection_grow(h, bad, 0, 1, C.byref(n)), "density_threshold")
        refused(lib.nrs_selection_grow(h, 0.01, 5, 1, C.byref(n)), "growing_level")
        refused(lib.nrs_selection_reset(h, None, 0, 5), "growing_level")
        seeds = np.array([3, 5 * VOL], np.uint32)
        refused(lib.nrs_selection_reset(h, seeds.ctypes.data, 2, 0), "h_cells[1]")
        refused(lib.nrs_selection_reset(h, None, 2, 0), "h_cells")
        for args, word in (((2, 2, 1, 2), "dilation: se_type"), ((0, 0, 1, 2), "dilation: radius"), ((0, 11, 1, 2), "dilation: radius"), ((0, 2, -1, 2), "erosion: se_type"),
                           ((0, 2, 1, 0), "erosion: radius"), ((0, 2, 1, 11), "erosion: radius")):
            refused(lib.nrs_selection_set_structuring_elements(h, *args), word)
        assert lib.nrs_selection_set_structuring_elements(h, 1, 10, 0, 1) == 0
        refused(lib.nrs_selection_state(None, None, None, None, None), "sel")
    finally:
        lib.nrs_selection_destroy(h)
    a, b = np.zeros(ref.BITFIELD_BYTES, np.uint8), np.zeros(ref.BITFIELD_BYTES, np.uint8)
    morph = lib.nrs_bitfield_morph_host
    refused(morph(None, 0, 0, 0, 1, b.ctypes.data), "h_in")
    refused(morph(a.ctypes.data, 0, 0, 0, 1, None), "h_out")
    refused(morph(a.ctypes.data, 5, 0, 0, 1, b.ctypes.data), "level")
    refused(morph(a.ctypes.data, 0, 2, 0, 1, b.ctypes.data), "op")
    refused(morph(a.ctypes.data, 0, 0, 2, 1, b.ctypes.data), "se_type")
    refused(morph(a.ctypes.data, 0, 0, 0, 0, b.ctypes.data), "radius")
    refused(morph(a.ctypes.data, 0, 0, 0, 11, b.ctypes.data), "radius")
    refused(morph(a.ctypes.data, 0, 0, 0, 1, a.ctypes.data), "overlaps")
    # the device entry point refuses the same before it touches a device (a NULL context first)
    refused(lib.nrs_bitfield_morph(None, None, a.ctypes.data, 0, 0, 0, 1, b.ctypes.data), "ctx")
    refused(lib.nrs_selection_dilate(None, None, None), "ctx")
    refused(lib.nrs_selection_fine_mesh(None, None, None, 1, None), "ctx")


def test_header_and_exports_name_the_new_entry_points(built):
    import os
    from nerfshop_amd import _abi
    lib = _abi.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nrs.h")).read()
    for name in ("nrs_selection_create", "nrs_selection_destroy", "nrs_selection_reset", "nrs_selection_grow", "nrs_selection_upscale", "nrs_selection_state",
                 "nrs_selection_get_cells", "nrs_selection_get_bitfield", "nrs_selection_set_structuring_elements", "nrs_bitfield_morph", "nrs_bitfield_morph_host",
                 "nrs_selection_dilate", "nrs_selection_erode", "nrs_selection_fine_mesh"):
        assert name in _abi.EXPORTS and hasattr(lib, name) and f"{name}(" in header, name
    assert lib.nrs_abi_version() == 3
