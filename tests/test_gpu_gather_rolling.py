"""The render kernel's rolling gather (nrs_hashgrid.cuh rolling_eval_sixteen) is another ORDER of the same loads and the same arithmetic: a frame rendered through it
must equal, bit for bit, the frame rendered through the loop over level pairs it stands beside.

The default cell-cache budget gives base.json's table the plan the rolling gather serves (levels 0..11 records, 12..15 hashed); a model without records
(set_cell_cache(0)) takes the loop for every level, and records hold the very entries the native gathers fetch (tests/test_gpu_cell_cache.py).  So every test renders one
small frame with the default plan and with no records and compares frame, depth, step counts and the sample count as words:

  * 64 x 40 with and without the cage edit in one-lane generations -- with the edit some waves have a warped sample outside the unit cube and take the loop in mid-frame;
  * a width and a height that are no multiples of 8 on the automatic schedule: a frame this small ends on teams of 2 and 4 lanes, tail packets and the hand-over, i.e.
    partial waves and idle lanes, whose features (not zeroed in the render kernel's rounds) must never reach a result;
  * tiny-cuda-nn's other roundings, whose instantiations gather the same way;
  * a two-sample batch (the BATCH twin);
  * budgets that end the records at other levels: whichever path such a plan takes, the picture is the same;
  * and the 64 x 40 frame of the default plan against the oracle, at the tolerances of tests/test_gpu_parity.py."""
import ctypes as C

import numpy as np
import pytest

from nerfshop_amd import _abi
from test_gpu_parity import _compare_frames
from test_gpu_spp_batch import batch_render

pytestmark = pytest.mark.gpu

DEFAULT_BUDGET = 10 << 30
ONE_LANE = -4  # nrs_ctx_set_lane_teams: the small-launch schedule with one lane on a pixel (generations of one lane per ray)


def _words(result):
    frame, depth, steps, stats = result
    return frame.view(np.uint32), depth.view(np.uint32), steps, int(stats.n_samples)


def _assert_same(got, ref, what):
    for a, b, name in zip(got[:3], ref[:3], ("frame", "depth", "steps")):
        assert np.array_equal(a, b), f"{what}: {name} differs in {int((a != b).sum())} words"
    assert got[3] == ref[3], (what, got[3], ref[3])


def _both_plans(rig, render, budgets=(DEFAULT_BUDGET,)):
    """-> (the no-records result, [the result under each budget]); leaves the default budget behind"""
    try:
        rig.net.set_cell_cache(0)
        assert rig.net.cell_cache()[1] == 0
        ref = render()
        got = []
        for b in budgets:
            rig.net.set_cell_cache(b)
            got.append(render())
    finally:
        rig.net.set_cell_cache(DEFAULT_BUDGET)
    assert rig.net.cell_cache()[1] == 12  # the plan of the rolling gather: twelve record levels, four hashed ones behind them
    return ref, got


@pytest.fixture()
def schedule(rig):
    def use(edit, teams):
        rig.use_edit(edit)
        rig.ctx.set_lane_teams(teams)
    yield use
    rig.ctx.set_lane_teams(0)
    rig.use_edit(False)


@pytest.mark.parametrize("edit", [False, True])
def test_frame_in_one_lane_generations(rig, schedule, edit):
    schedule(edit, ONE_LANE)
    p = rig.scene.params_for(64, 40, 60.0)
    ref, (got,) = _both_plans(rig, lambda: _words(rig.render(p)))
    assert ref[3] > 3000
    _assert_same(got, ref, f"64x40, edit {edit}")
    if edit:  # the edit is in the picture: warped samples, some of them outside the unit cube
        p0 = rig.scene.params_for(64, 40, 60.0, apply_operators=False)
        assert not np.array_equal(_words(rig.render(p0))[0], got[0])


def test_odd_frame_on_the_automatic_schedule(rig, schedule):
    schedule(True, 0)
    p = rig.scene.params_for(61, 37, 60.0)
    ref, (got,) = _both_plans(rig, lambda: _words(rig.render(p)))
    assert ref[3] > 3000
    _assert_same(got, ref, "61x37, automatic schedule")


@pytest.mark.parametrize("grid_acc,mlp_acc", [(1, 1), (1, 0), (0, 1)])
def test_tcnn_roundings(rig, schedule, grid_acc, mlp_acc):
    schedule(True, 0)
    p = rig.scene.params_for(64, 40, 60.0)
    try:
        rig.net.set_numerics(grid_acc, mlp_acc)
        ref, (got,) = _both_plans(rig, lambda: _words(rig.render(p)))
    finally:
        rig.net.set_numerics(0, 0)
    assert ref[3] > 3000
    _assert_same(got, ref, f"64x40, numerics ({grid_acc}, {mlp_acc})")


def test_two_sample_batch(rig, schedule):
    schedule(True, 0)
    p = rig.scene.params_for(64, 40, 60.0)
    ref, (got,) = _both_plans(rig, lambda: batch_render(rig, p, 3, 2, 0))
    assert ref[3][0] > 6000
    assert not np.array_equal(ref[0][0], ref[0][1])  # two different samples of the pixel
    for a, b, name in zip(got[:3], ref[:3], ("frame", "depth", "steps")):
        assert np.array_equal(a, b), f"two-sample batch: {name} differs in {int((a != b).sum())} words"
    assert got[3] == ref[3]


def test_other_record_budgets(rig, schedule):
    res = (C.c_uint32 * 16)()
    _abi.check(_abi.load().nrs_model_level_table(C.byref(rig.scene.desc), None, res, None, None, None))
    cells = [int(r) ** 3 for r in res]
    schedule(True, 0)
    p = rig.scene.params_for(64, 40, 60.0)
    plans = []

    def render():
        plans.append(rig.net.cell_cache()[1])
        return _words(rig.render(p))
    ref, got = _both_plans(rig, render, budgets=(32 * sum(cells[:8]), 32 * sum(cells[:10]), 32 * sum(cells[:11])))
    assert plans == [0, 8, 10, 10], plans  # (an odd number of levels is rounded down to whole pairs: plan_cell_cache)
    for g, n in zip(got, plans[1:]):
        _assert_same(g, ref, f"64x40, records up to level {n - 1}")


def test_default_plan_against_the_oracle(rig, schedule):
    schedule(True, 0)
    assert rig.net.cell_cache()[1] == 12
    p = rig.scene.params_for(64, 40, 60.0)
    frame, depth, steps, stats = rig.render(p)
    ref_frame, ref_depth, ref_steps, ref_stats = rig.scene.oracle_model.render(p, [rig.scene.oracle_edit])
    assert ref_stats.n_hit > 100
    _compare_frames(frame, depth, steps, ref_frame, ref_depth, ref_steps)
