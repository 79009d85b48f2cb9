"""The occupancy refresh as training drives it (Trainer.update_density_grid -> nrs_model_update_density_grid: grid_refresh_kernel, grid_ema_kernel, mean, bitfield,
mips, marching accelerator) against the oracle, in the states tests/test_gpu_grid_refresh.py does not reach: grids with untrained (-1) cells, where the sampler's
retry loop works and gives up; the cell-order path with several cascades and a non-uniform draw behind it; ema_step far from 0, up to the uint32 wrap of
step * n; cell order against sample order, byte for byte; the value regimes of the Trainer's start weights and of tests/value_regimes.py's `large` and `overflow`;
and the fields, counts and generator states the Trainer hands over on both sides of step 256.  Inputs and their preconditions: tests/occupancy_ref.py, pinned
without a GPU by tests/test_occupancy_training_host.py.  Measured figures and the mutants these tests were run against: profiles/occupancy_training.md.

One rule for every comparison: both sides start the compared call from the same bytes (set_density_grid(start) on the device, a copy of `start` for the oracle),
with the same GridUpdate fields, and one call is made on each side -- the non-uniform draw chooses cells by grid > 0.01, so a 1-ulp difference carried over from an
earlier call would move samples to other cells, which is no error of the call under test.

Bars.  The state (ema_step, rng) and the SET of cells written are exact.  Values: test_gpu_grid_refresh's bar (its docstring derives rtol 1e-2, atol 1e-7 from one
fp16 ulp of the raw density; >= 99 % of the cells bit-identical), through its own _compare where the oracle's bitfield is compared too.  The bitfield, the mips and
the threshold are integer / order-controlled work on the DEVICE's grid: the device's bitfield is byte-equal to the oracle's grid -> bitfield of the device's grid,
whatever number of cells sit at the threshold.  A bit of the oracle's OWN bitfield may differ only where the oracle's value lies within 1.5 % of the threshold.
Cells beyond max_cascade are not sampled but the ema pass still runs over them (ema_grid_samples_nerf covers all five cascades): byte-equal to the oracle's, which
is `start` where start <= 0 and float32(start * decay) elsewhere."""
import os
import subprocess
import sys
import time
from types import SimpleNamespace

import numpy as np
import pytest

import occupancy_ref as oref
from occupancy_ref import CASES, VOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def oracle(rig_shaped, rig16_shaped):
    return oref.Oracle(rig_shaped.scene, rig16_shaped.scene)


@pytest.fixture(scope="module")
def nets(rig_shaped, rig16_shaped, oracle):
    """scene name of a case -> the network that holds its parameters: the rigs' own for the shaped scenes, one NerfNetwork per regime blob"""
    from nerfshop_amd import runtime
    made = {"shaped": rig_shaped.net, "shaped16": rig16_shaped.net}

    def get(name):
        if name not in made:
            net = runtime.NerfNetwork(rig_shaped.ctx, oracle.desc, cell_cache_bytes=0)
            net.set_params(oracle.params(name))
            made[name] = net
        return made[name]
    yield get
    for rig in (rig_shaped, rig16_shaped):   # the rigs' occupancy as the other modules expect it
        rig.use_edit(False)


def check_refresh(label, got_grid, got_bits, accel, u, u_ref, start, decay, ref_grid, ref_bits, n_cascades, oracle_bits, min_share):
    """The assertions of one compared call.  `accel`: which -> (box12, mask bits) of the marching accelerator that belongs to got_bits.  Prints the measured figures
    before it asserts and returns them."""
    from oracle import oracle as orc
    from test_gpu_grid_refresh import _compare
    from test_gpu_march_accelerator import _check
    n = VOL * n_cascades
    g, r = got_grid[:n], ref_grid[:n]
    same = float((g.view(np.uint32) == r.view(np.uint32)).mean())
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        rel = np.abs(g.astype(np.float64) - r) / np.maximum(np.abs(r.astype(np.float64)), 1e-30)
        worst_rel = float(np.nanmax(np.where(np.isfinite(rel), rel, 0.0)))
    own_bits = orc.density_grid_to_bitfield(got_grid)
    diff_own = int((np.unpackbits(got_bits) != np.unpackbits(own_bits)).sum())
    diff = np.unpackbits(got_bits, bitorder="little") != np.unpackbits(ref_bits, bitorder="little")
    figures = dict(case=label, samples=int(u_ref.n_uniform_samples + u_ref.n_nonuniform_samples), share_identical=same, worst_rel=worst_rel,
                   bits_vs_oracle=int(diff.sum()), bits_vs_own_grid=diff_own, bits_set_cascade0=int(np.unpackbits(got_bits[:VOL // 8]).sum()))
    print("occupancy_training figures:", figures)
    # state
    assert (u.ema_step, u.rng_state, u.rng_inc) == (u_ref.ema_step, u_ref.rng_state, u_ref.rng_inc)
    # cells that are not sampled, cells that are untrained
    assert got_grid[n:].tobytes() == ref_grid[n:].tobytes()
    rest = start[n:]
    with np.errstate(invalid="ignore"):
        assert got_grid[n:].tobytes() == np.where(rest <= 0, rest, rest * np.float32(decay)).astype(np.float32).tobytes()
    assert np.array_equal(ref_grid[start < 0], start[start < 0])
    assert got_grid[start < 0].tobytes() == start[start < 0].tobytes(), "an untrained cell changed"
    # the set of cells written, the class of every value, the values
    assert np.array_equal(g == 0, r == 0), "different set of cells written"
    assert np.array_equal(np.isposinf(g), np.isposinf(r)) and np.array_equal(np.isneginf(g), np.isneginf(r)) and np.array_equal(np.isnan(g), np.isnan(r))
    assert same >= min_share, f"only {same:.4f} of the cells bit-identical"
    np.testing.assert_allclose(g, r, rtol=1e-2, atol=1e-7)
    # the bitfield: exact on the device's own grid
    assert oref.tree_mean(got_grid).tobytes() == oref.sequential_mean(got_grid).tobytes(), "the two summation orders round this grid's mean differently"
    assert diff_own == 0, f"{diff_own} bits differ from the oracle's bitfield of the device's grid"
    # ... and against the oracle's own only near the threshold
    bad0 = np.nonzero(diff[:VOL])[0]
    thresh = oref.threshold(ref_grid)
    assert np.all(np.abs(ref_grid[bad0] - thresh) <= 1.5e-2 * thresh), "bitfield differs from the oracle's away from the threshold"
    view = SimpleNamespace(get_density_grid=lambda: got_grid, get_density_bitfield=lambda: got_bits, get_march_accelerator=accel)
    if oracle_bits:
        _compare(SimpleNamespace(net=view), SimpleNamespace(orc=orc), u, u_ref, ref_grid, ref_bits, n_cascades)
    _check(view, got_bits)
    return figures


def run_case(nets, oracle, name):
    case = CASES[name]
    net = nets(case["scene"])
    start = oracle.start(case["start"])
    t0 = time.perf_counter()
    u_ref, ref_grid, ref_bits = oracle.run(name)
    t_oracle = time.perf_counter() - t0
    net.set_density_grid(start)
    u = oref.grid_update(case)
    net.update_density_grid(u)
    got_grid, got_bits = net.get_density_grid(), net.get_density_bitfield()
    print(f"occupancy_training oracle seconds: {name} {t_oracle:.2f}")
    return check_refresh(name, got_grid, got_bits, net.get_march_accelerator, u, u_ref, start, case["decay"], ref_grid, ref_bits, case["max_cascade"] + 1,
                         case["oracle_bits"], case["min_share"])


def test_untrained_cells_cell_order(nets, oracle):
    """A: 2^21 uniform samples walk the cells in Morton order over a grid half of whose 4x4x4 blocks are untrained: every depth of the retry loop, 1654 samples
    that exhaust it (they land on a -1 cell, which grid_ema_kernel keeps)"""
    run_case(nets, oracle, "A")


@pytest.mark.parametrize("name", ["B", "B_ragged"])
def test_untrained_cells_sample_order_with_step_offset(nets, oracle, name):
    """B: 2^19 + 2^19 samples at ema_step 17 (the Trainer's counts after step 256): sample order, the step term in every cell index, the non-uniform draw from the
    generator advanced by 2^32 over a grid where most of its samples find no cell above 0.01; ragged counts put both draws into one wave"""
    run_case(nets, oracle, name)


@pytest.mark.parametrize("name", ["C", "C_wrap"])
def test_cascades_without_an_edit(nets, oracle, name):
    """C: max_cascade 3, 2^21 uniform samples in cell order with a random level each and a non-uniform draw behind them; C_wrap: step * n past 2^32"""
    figures = run_case(nets, oracle, name)
    case, start, ref_grid = CASES[name], oracle.start(CASES[name]["start"]), oracle.run(name)[1]
    for level in range(case["max_cascade"] + 1):   # from the oracle's side: every sampled cascade received values
        assert (ref_grid[level * VOL:(level + 1) * VOL] > start[level * VOL:(level + 1) * VOL]).sum() > 1000
    assert figures["samples"] == oref.n_samples(case)


@pytest.mark.parametrize("name", ["E_initial", "E_large", "E_overflow", "E_initial_dense", "E_initial_untrained"])
def test_value_regimes(nets, oracle, name):
    """E: the Trainer's start weights (every thickness the same: the threshold is the mean, and in E_initial_dense every cell EQUALS it), `large` (threshold 0.01,
    values 100 times the Trainer's) and `overflow` (exp leaves fp16: +inf cells, an infinite mean, NaN thicknesses that fmaxf drops)"""
    figures = run_case(nets, oracle, name)
    ref_grid = oracle.run(name)[1]
    if name == "E_overflow":
        assert np.isinf(ref_grid[:VOL]).sum() > 100
    if name == "E_initial_dense":
        assert figures["bits_set_cascade0"] == 0
    if name == "E_initial_untrained":
        assert 0.1 * VOL < figures["bits_set_cascade0"] < 0.9 * VOL


def test_cell_order_equals_sample_order(nets, oracle, tmp_path):
    """D: A and C again in a child process with NRS_DEV_KNOBS=1 NRS_REFRESH_ORDER=0 (the kernel walks the samples in their own order and takes i as it comes):
    grid and bitfield byte-equal to this process's, which inverts the sample -> cell map (i = Kinv * (cell - C), the wrap table, the composed generator skips)"""
    knobs_on = os.environ.get("NRS_DEV_KNOBS", "")[:1] not in ("", "0")
    assert not (knobs_on and "NRS_REFRESH_ORDER" in os.environ), "this process must run the default order"
    for name in oref.WORKER_CASES:
        np.save(os.path.join(tmp_path, f"start_{name}.npy"), oracle.start(CASES[name]["start"]))
    env = dict(os.environ, NRS_DEV_KNOBS="1", NRS_REFRESH_ORDER="0")
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "occupancy_worker.py"), str(tmp_path)], env=env, stdout=subprocess.PIPE,
                        stderr=subprocess.PIPE, text=True, timeout=300)
    assert pr.returncode == 0, (pr.stdout[-2000:], pr.stderr[-4000:])
    assert "refreshes in sample order: %d" % len(oref.WORKER_CASES) in pr.stdout, pr.stdout[-2000:]
    for name in oref.WORKER_CASES:
        case = CASES[name]
        net = nets(case["scene"])
        net.set_density_grid(oracle.start(case["start"]))
        u = oref.grid_update(case)
        net.update_density_grid(u)
        child = np.load(os.path.join(tmp_path, f"out_{name}.npz"))
        grid, bits = net.get_density_grid(), net.get_density_bitfield()
        n_diff = int((grid.view(np.uint32) != child["grid"].view(np.uint32)).sum())
        print(f"occupancy_training figures: {name} cell order vs sample order: {n_diff} cells differ")
        assert (grid != oracle.start(case["start"])).sum() > 100000
        assert grid.tobytes() == child["grid"].tobytes(), f"{name}: {n_diff} cells differ between cell order and sample order"
        assert bits.tobytes() == child["bits"].tobytes()
        assert [int(v) for v in child["state"]] == [u.ema_step, u.rng_state, u.rng_inc]


# ---- F: the Trainer's cadence ------------------------------------------------------------------------------------------------------------------------
def _spied(records, run):
    """NerfNetwork.update_density_grid that records the fields handed over, the grid before and everything derived after; run=False records the fields only"""
    from nerfshop_amd import runtime
    real = runtime.NerfNetwork.update_density_grid

    def spy(self, update, edit_operators=(), stream=None):
        rec = dict(before=oref.copy_update(update), n_edits=len(edit_operators))
        if run:
            rec["start"] = self.get_density_grid()
            real(self, update, edit_operators, stream)
            accel = [self.get_march_accelerator(which) for which in (0, 1)]
            rec.update(after=oref.copy_update(update), grid=self.get_density_grid(), bits=self.get_density_bitfield(), accel=accel)
        records.append(rec)
    return real, spy


@pytest.fixture(scope="module")
def trainer_calls(rig_shaped):
    """Trainer(seed=11) without a grid: the constructor's own update_density_grid, then one call each at training step 16, 256 and 272 (no training steps: the weights
    stay the Trainer's start weights, which the oracle shares)"""
    from nerfshop_amd import _abi, runtime, synth
    from nerfshop_amd.trainer import Trainer
    records = []
    real, spy = _spied(records, run=True)
    runtime.NerfNetwork.update_density_grid = spy
    try:
        trainer = Trainer(rig_shaped.ctx, synth.model_desc(1), seed=oref.TRAINER_SEED)
        for step, *_ in oref.TRAINER_CALLS[1:]:
            trainer.training_step = step
            trainer.update_density_grid()
    finally:
        runtime.NerfNetwork.update_density_grid = real
    params = trainer.optimizer.export_fp16(_abi.OPT_EXPORT_WEIGHTS).cpu().numpy().view(np.uint16)
    return SimpleNamespace(records=records, params=params, ema_step=trainer._grid_update.ema_step)


def test_trainer_hands_over_the_table(trainer_calls):
    from oracle import oracle as orc
    recs = trainer_calls.records
    assert len(recs) == len(oref.TRAINER_CALLS) and trainer_calls.ema_step == 4
    rng = orc.Pcg32(oref.TRAINER_SEED)
    for rec, (step, n_uni, n_non, k, ema_step) in zip(recs, oref.TRAINER_CALLS):
        b, a = rec["before"], rec["after"]
        assert (b.n_uniform_samples, b.n_nonuniform_samples) == (n_uni, n_non), step
        assert b.decay == float(np.float32(0.95 ** (k / 16))), step
        assert (b.reset_grid, b.max_cascade, b.ema_step, rec["n_edits"]) == (0, 0, ema_step, 0), step
        assert (b.rng_state, b.rng_inc) == (rng.state.value, rng.inc.value), step
        rng.advance(2 << 32)
        assert (a.rng_state, a.rng_inc, a.ema_step) == (rng.state.value, rng.inc.value, ema_step + 1), step
    assert recs[0]["start"].tobytes() == bytes(4 * 5 * VOL), "a new network's grid is empty"
    for prev, rec in zip(recs, recs[1:]):
        assert rec["start"].tobytes() == prev["grid"].tobytes()


@pytest.mark.parametrize("k", range(len(oref.TRAINER_CALLS)))
def test_trainer_call_matches_oracle(trainer_calls, oracle, k):
    """each of the Trainer's calls replayed in the oracle from the bytes the device started from: calls 0 and 1 fill every cell with the same thickness (the grid equals
    its mean: an empty bitfield), call 2 decays by 0.95^15 and re-samples a quarter (the non-uniform draw finds no cell above 0.01 and takes its tenth cell each time),
    call 3 does so again on a grid of three values"""
    assert np.array_equal(trainer_calls.params, oracle.params("initial")), "the Trainer's weights are initial_params(n, 11) rounded to fp16"
    rec = trainer_calls.records[k]
    u_ref, ref_grid = oref.copy_update(rec["before"]), rec["start"].copy()
    t0 = time.perf_counter()
    ref_bits = oracle.refresh("initial", ref_grid, u_ref)
    print(f"occupancy_training oracle seconds: F{k} {time.perf_counter() - t0:.2f}")
    figures = check_refresh(f"F{k}", rec["grid"], rec["bits"], lambda which: rec["accel"][which], rec["after"], u_ref, rec["start"], rec["before"].decay, ref_grid,
                            ref_bits, 1, False, 0.99)
    if k < 2:
        assert figures["bits_set_cascade0"] == 0 and np.unique(rec["grid"][:VOL]).size == 1
    else:
        assert 0.1 * VOL < figures["bits_set_cascade0"] < 0.9 * VOL and np.unique(rec["grid"][:VOL]).size == k


def test_trainer_counts_with_four_cascades(rig_shaped):
    """max_cascade 3: every cell of four cascades below step 256, 2^21 + 2^21 from then on (the cell-order path with a second draw behind it: case C).  The calls are
    recorded, not run."""
    from nerfshop_amd import runtime, synth
    from nerfshop_amd.trainer import Trainer
    records = []
    real, spy = _spied(records, run=False)
    runtime.NerfNetwork.update_density_grid = spy
    try:
        trainer = Trainer(rig_shaped.ctx, synth.model_desc(1), seed=oref.TRAINER_SEED, max_cascade=3)
        trainer.training_step = 256
        trainer.update_density_grid()
    finally:
        runtime.NerfNetwork.update_density_grid = real
    assert len(records) == 2
    for rec, (step, n_uni, n_non) in zip(records, oref.TRAINER_CALLS_CASCADE3):
        b = rec["before"]
        assert (b.n_uniform_samples, b.n_nonuniform_samples, b.max_cascade, b.reset_grid) == (n_uni, n_non, 3, 0), step
    assert records[0]["before"].decay == float(np.float32(0.95)) and records[1]["before"].decay == float(np.float32(0.95 ** 16))
