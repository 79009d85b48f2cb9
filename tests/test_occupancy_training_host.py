"""tests/occupancy_ref.py without a GPU: the inputs of tests/test_gpu_occupancy_training.py are pinned against the oracle alone, so that the GPU tests cannot pass
vacuously -- the retry loop's every depth is populated, the sampler restatement chooses the cells the oracle writes, the device's summation order and the oracle's
round every grid's mean to the same float32 (what the byte-equal bitfield rule rests on), the 64-bit allowance can hold where it is used, and the value regimes
are the regimes they are named after."""
import numpy as np
import pytest

import occupancy_ref as oref
from occupancy_ref import CASES, VOL


@pytest.fixture(scope="module")
def oracle(built, scene_shaped, scene16_shaped):
    return oref.Oracle(scene_shaped, scene16_shaped)


def _cascade(grid, level):
    return grid[level * VOL:(level + 1) * VOL]


def test_case_table_takes_each_path():
    """the arithmetic that routes each case inside grid_refresh_kernel: cell order needs n_uniform = 0 mod 2^21; B's step term; the ragged counts; the 2^32 wrap"""
    a, b, br, c, cw = (CASES[k] for k in ("A", "B", "B_ragged", "C", "C_wrap"))
    assert a["n_uniform"] % VOL == 0 and a["n_nonuniform"] == 0 and a["max_cascade"] == 0
    assert b["n_uniform"] % VOL != 0 and (b["ema_step"] * b["n_uniform"]) % VOL == 1 << 19 and b["n_nonuniform"] == b["n_uniform"]
    assert br["n_uniform"] % 64 == 37 and oref.n_samples(br) % 64 != 0           # one wave holds samples of both draws; the last tile is not full
    assert c["n_uniform"] % VOL == 0 and c["max_cascade"] == 3 and c["n_nonuniform"] % 64 != 0
    assert cw["ema_step"] * cw["n_uniform"] > 1 << 32 and cw["n_uniform"] % VOL != 0 and cw["max_cascade"] == 2
    assert all(CASES[k]["start"] in ("untrained", "untrained16") for k in ("A", "B", "B_ragged", "C", "C_wrap"))
    # the Trainer's counts: every cell below step 256, a quarter and a quarter from then on
    for cascades, table in ((1, [t[:3] for t in oref.TRAINER_CALLS]), (4, oref.TRAINER_CALLS_CASCADE3)):
        for step, n_uni, n_non in table:
            assert (n_uni, n_non) == ((cascades * VOL, 0) if step < 256 else (cascades * VOL // 4, cascades * VOL // 4))
    assert oref.TRAINER_CALLS_CASCADE3[1][1] % VOL == 0       # max_cascade 3 after step 256: the cell-order path with a second draw behind it (case C)
    assert oref.TRAINER_CALLS[2][1] % VOL != 0                # max_cascade 0 after step 256: sample order with a step offset (case B)


def test_untrained_grid_marks_whole_blocks(oracle):
    for name in ("untrained", "untrained16", "zeros_untrained"):
        g = oracle.start(name)
        neg = (g < 0).reshape(-1, 64)
        assert np.array_equal(neg.all(1), neg.any(1)), "a 4x4x4 block is untrained as a whole"
        assert (g[g < 0] == -1.0).all()
        for level in range(5):
            assert 0.48 < (_cascade(g, level) < 0).mean() < 0.52
    base = np.arange(5 * VOL, dtype=np.float32)
    again = oref.untrained_grid(base, 3)
    assert np.array_equal(again < 0, oracle.start("untrained") < 0) and np.array_equal(again[again >= 0], base[again >= 0])
    assert not np.array_equal(oref.untrained_grid(base, 4) < 0, again < 0)
    # the start grids hold what the draws need: values above the non-uniform threshold to find, in every cascade that is sampled
    assert (_cascade(oracle.start("untrained"), 0) > 0.01).sum() > 1000
    for level in range(5):
        assert (_cascade(oracle.start("untrained16"), level) > 0.01).sum() > 1000


@pytest.mark.parametrize("name", ["A", "B"])
def test_retry_loop_is_exercised_at_every_depth(oracle, name):
    """every try count 1..10 occurs in the uniform draw and at least 100 samples exhaust all ten tries (measured: A 1654 of 2^21, B 432 of 2^19)"""
    case = CASES[name]
    start = _cascade(oracle.start(case["start"]), 0)
    cell, tries, exhausted = oref.sample_cells(start, case["n_uniform"], case["ema_step"], oref.UNIFORM_THRESH)
    counts = np.bincount(tries, minlength=11)
    assert counts[0] == 0 and (counts[1:11] > 0).all(), counts
    assert exhausted.sum() >= 100
    assert (start[cell[exhausted]] < 0).all() and (start[cell[~exhausted]] >= 0).all()
    if case["n_nonuniform"]:
        # the second draw looks for cells above 0.01: most samples run the loop to its end, some find one early
        _, tries2, exhausted2 = oref.sample_cells(start, case["n_nonuniform"], case["ema_step"], oref.NONUNIFORM_THRESH)
        assert (np.bincount(tries2, minlength=11)[1:11] > 100).all() and 0.5 < exhausted2.mean() < 0.95


def test_step_term_moves_the_samples(oracle):
    """B's ema_step changes the cells chosen (dropped, the first try of sample i would be cell i * K + C)"""
    case = CASES["B"]
    start = _cascade(oracle.start(case["start"]), 0)
    with_step = oref.sample_cells(start, case["n_uniform"], case["ema_step"], oref.UNIFORM_THRESH)[0]
    without = oref.sample_cells(start, case["n_uniform"], 0, oref.UNIFORM_THRESH)[0]
    assert (with_step != without).mean() > 0.99
    # C_wrap: the product wraps past 2^32 as a uint32 (a 64-bit product would choose other cells)
    cw = CASES["C_wrap"]
    offset = (cw["ema_step"] * cw["n_uniform"]) % (1 << 32)
    want = [(((i + offset) % (1 << 32)) * oref.SAMPLE_MUL + oref.SAMPLE_ADD) % (1 << 32) % VOL for i in range(8)]   # in Python's integers
    got = oref.sample_cells(np.zeros(VOL, np.float32), cw["n_uniform"], cw["ema_step"], oref.UNIFORM_THRESH)[0][:8]
    assert got.tolist() == want


def test_restatement_chooses_the_cells_the_oracle_writes(oracle):
    """A's draw on a grid that keeps only the untrained cells of A's start (everything else 0): the cells that hold a value afterwards are the restatement's chosen
    cells minus the negative ones (an exhausted sample's cell is negative and stays -1)"""
    case = CASES["A"]
    start = np.where(oracle.start(case["start"]) < 0, np.float32(-1), np.float32(0)).astype(np.float32)
    grid = start.copy()
    oracle.refresh(case["scene"], grid, oref.grid_update(case))
    cell, tries, exhausted = oref.sample_cells(start[:VOL], case["n_uniform"], case["ema_step"], oref.UNIFORM_THRESH)
    want = np.zeros(VOL, bool)
    want[cell[~exhausted]] = True
    assert not (want & (start[:VOL] < 0)).any()
    assert np.array_equal(grid[:VOL] > 0, want)
    assert np.array_equal(grid[VOL:], start[VOL:]) and np.array_equal(grid[start < 0], start[start < 0])
    # the retries land two samples in one cell: fewer cells written than samples that found one
    assert 0.3 * VOL < want.sum() < (~exhausted).sum()


def test_mean_restatements():
    """tree_mean is the device's order and sequential_mean the oracle's: numpy's mean within one float32 ulp, the oracle's own threshold exactly"""
    rng = np.random.default_rng(0)
    g = np.zeros(5 * VOL, np.float32)
    g[:VOL] = rng.random(VOL, dtype=np.float32) - np.float32(0.25)
    want = np.maximum(g[:VOL], 0).astype(np.float64).mean()
    assert abs(float(oref.tree_mean(g)) - want) <= 2.0 ** -23 * want and abs(float(oref.sequential_mean(g)) - want) <= 2.0 ** -23 * want
    from oracle import oracle as orc
    assert oref.threshold(g) == np.float32(orc.load().orc_density_grid_threshold(g.ctypes.data)) == np.float32(0.01)
    g[:VOL] *= np.float32(0.01)
    assert oref.threshold(g) == np.float32(orc.load().orc_density_grid_threshold(g.ctypes.data)) == oref.sequential_mean(g)
    g[:] = -1.0
    assert oref.tree_mean(g) == 0 and oref.sequential_mean(g) == 0
    g[5] = np.inf
    assert oref.tree_mean(g) == np.inf and oref.sequential_mean(g) == np.inf


@pytest.mark.parametrize("name", sorted(CASES))
def test_both_summation_orders_round_the_mean_alike(oracle, name):
    """for every start grid and every oracle result of the GPU cases: the device's two-stage tree and the oracle's running sum give the same float32"""
    start = oracle.start(CASES[name]["start"])
    _, grid, bits = oracle.run(name)
    for g in (start, grid):
        assert oref.tree_mean(g).tobytes() == oref.sequential_mean(g).tobytes()
    from oracle import oracle as orc
    assert np.array_equal(bits, orc.density_grid_to_bitfield(grid))


@pytest.mark.parametrize("name", ["A", "B", "B_ragged", "C", "C_wrap"])
def test_bit_allowance_can_hold_where_it_is_used(oracle, name):
    """test_gpu_grid_refresh._compare lets at most 64 bits differ, each within 1.5 % of the threshold: on the oracle's side no more than 64 cells of cascade 0 may lie
    that close, or the GPU test does not use the allowance for the case (occupancy_ref.CASES: oracle_bits)"""
    _, grid, _ = oracle.run(name)
    near = oref.near_threshold_cells(grid)
    print(f"{name}: {near} cells of cascade 0 within 1.5 % of the threshold {oref.threshold(grid)!r}")
    assert CASES[name]["oracle_bits"] == (near <= 64)


@pytest.mark.parametrize("name", ["C", "C_wrap"])
def test_every_sampled_cascade_receives_values(oracle, name):
    case = CASES[name]
    start = oracle.start(case["start"])
    _, grid, _ = oracle.run(name)
    share = oref.n_samples(case) / ((case["max_cascade"] + 1) * VOL)
    for level in range(5):
        raised = (_cascade(grid, level) > _cascade(start, level)).sum()
        if level <= case["max_cascade"]:
            assert raised > 0.2 * share * VOL, (level, raised)      # (half the cells are untrained, some samples share a cell, some lose against prev * decay)
        else:
            assert raised == 0
            s, g = _cascade(start, level), _cascade(grid, level)
            assert np.array_equal(g, np.where(s < 0, s, s * np.float32(case["decay"])))   # the ema pass still decays them
    assert np.array_equal(grid[start < 0], start[start < 0])


def test_regime_facts(oracle):
    """what each blob of case E does to the grid, from the oracle"""
    from nerfshop_amd import synth
    thickness = np.float32(1.0) * np.float32(synth.MIN_STEP)
    facts = {}
    for name in ("E_initial", "E_large", "E_overflow", "E_initial_dense", "E_initial_untrained"):
        _, grid, bits = oracle.run(name)
        v = grid[:VOL]
        facts[name] = dict(inf=int(np.isinf(v).sum()), nan=int(np.isnan(v).sum()), written=int((v > 0).sum()), threshold=float(oref.threshold(grid)),
                           mean=float(oref.sequential_mean(grid)), bits=float(np.unpackbits(bits[:VOL // 8]).mean()))
        print(name, facts[name])
        assert not np.isnan(grid).any()   # fmaxf(prev * decay, NaN) keeps prev * decay: a NaN thickness never reaches the grid
        assert np.array_equal(grid[VOL:], oracle.start(CASES[name]["start"])[VOL:])
    # the Trainer's start: every density is fp16 1.0, the threshold is the mean
    for name in ("E_initial", "E_initial_dense", "E_initial_untrained"):
        _, grid, _ = oracle.run(name)
        f = facts[name]
        assert f["inf"] == 0 and f["threshold"] == f["mean"] < 0.01
        assert (grid[:VOL][grid[:VOL] > 0] == thickness).all()
    assert facts["E_initial"]["written"] > 0.9 * CASES["E_initial"]["n_uniform"] and facts["E_initial"]["bits"] == facts["E_initial"]["written"] / VOL
    # one sample per cell, no untrained cell: the mean EQUALS every cell, nothing lies above it (occupancy_ref.CASES' comment)
    assert facts["E_initial_dense"]["written"] == VOL and facts["E_initial_dense"]["mean"] == float(thickness) and facts["E_initial_dense"]["bits"] == 0.0
    # with untrained cells the mean drops below the thickness and the bitfield is dense
    assert 0.1 < facts["E_initial_untrained"]["bits"] < 0.9
    assert facts["E_initial_untrained"]["bits"] == facts["E_initial_untrained"]["written"] / VOL
    # large: finite values far above the Trainer's, threshold 0.01; overflow: exp leaves fp16 in some cells, the mean is inf and the threshold 0.01
    assert facts["E_large"]["inf"] == 0 and facts["E_large"]["threshold"] == float(np.float32(0.01)) and oracle.run("E_large")[1].max() > 50 * thickness
    assert facts["E_overflow"]["inf"] > 100 and facts["E_overflow"]["mean"] == np.inf and facts["E_overflow"]["threshold"] == float(np.float32(0.01))
    assert (oracle.run("E_overflow")[1][:VOL] == 0).sum() > (oracle.run("E_large")[1][:VOL] == 0).sum()   # NaN thicknesses are lost in fmaxf


def test_trainer_decay_table():
    """decay = 0.95^(k / 16) as the Trainer computes it and as a float32 field holds it"""
    import ctypes as C
    for step, _, _, k, _ in oref.TRAINER_CALLS:
        assert C.c_float(0.95 ** (k / 16.0)).value == float(np.float32(0.95 ** (k / 16)))
    assert np.float32(0.95 ** (240 / 16)) == np.float32(0.46329123015975304)
