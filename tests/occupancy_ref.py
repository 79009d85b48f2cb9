"""The occupancy refresh as training drives it, without a GPU: the grids, the sampler's cell choice and the device's mean restated, and the case table that
tests/test_gpu_occupancy_training.py (on an MI355X) and tests/test_occupancy_training_host.py (the same inputs against the oracle alone) both read.

Grid maker.  mark_untrained_density_grid writes -1 into cells no camera sees; untrained_grid does so to whole 4 x 4 x 4 blocks (64 consecutive Morton cells) of every
cascade, each with probability `share`: the sampler's retry loop (ten tries, j * 19349663 apart) then does work, and about share^10 of the samples exhaust it.

Sampler restatement (n_cascades == 1).  Sample i of a draw of n picks cell ((i + step * n) * 56924617 + j * 19349663 + 96925573) mod 2^32 mod 2^21 for the first
j in 0..9 whose cell lies above the threshold (-0.01 for the uniform draw, 0.01 for the non-uniform one), and the j = 9 cell if none does (common_nerf.cu:189-195).

Mean restatement.  The bitfield's threshold is min(0.01, mean of max(v, 0) / 2^21 over cascade 0).  The oracle adds the 2^21 terms one after the other in float64; the
device adds them in a fixed two-stage tree (256 blocks of 8192 contiguous cells, 256 strided partial sums per block, halving trees).  Both round to float32 at the end:
float64 carries 29 bits more than float32, so the two orders can differ only where the sum lies within ~2^-30 relative of a float32 rounding boundary.  The host test
asserts, grid by grid, that they do not: the byte-equal bitfield rule of the GPU tests rests on it."""
import numpy as np

VOL = 128 ** 3
CASCADES = 5
SAMPLE_MUL, SAMPLE_STEP, SAMPLE_ADD = 56924617, 19349663, 96925573
UNIFORM_THRESH, NONUNIFORM_THRESH = np.float32(-0.01), np.float32(0.01)
UNTRAINED_SEED = 3

# The refreshes compared with the oracle, each from its own start grid (Oracle.start below).  `oracle_bits`: the oracle's own bitfield is compared too, under
# test_gpu_grid_refresh._compare's allowance of 64 bits.  That allowance can only hold where at most 64 cells of cascade 0 lie within 1.5 % of the threshold on the
# oracle's side, which the host test asserts for these cases; B_ragged (68 such cells), C (400) and C_wrap (177) have more, so for them that comparison is dropped: there
# a bit of the oracle's may differ wherever its value lies within 1.5 % of the threshold, without a cap on the count.  The byte-equal rule (the device's bitfield
# against the oracle's grid -> bitfield of the DEVICE's grid) holds for every case.
# `min_share`: the share of bit-identical cells asserted (0.99: test_gpu_grid_refresh's bar; measured figures: profiles/occupancy_training.md).
CASES = {
    # A: untrained cells under the cell-order path (2^21 is the smallest count at which it exists)
    "A": dict(scene="shaped", start="untrained", max_cascade=0, n_uniform=1 << 21, n_nonuniform=0, ema_step=3, decay=0.95, seed=1337),
    # B: sample order, 17 * 2^19 mod 2^21 = 2^19: the step term moves every sample; the second run has one wave straddling the two draws and a ragged tail tile
    "B": dict(scene="shaped", start="untrained", max_cascade=0, n_uniform=1 << 19, n_nonuniform=1 << 19, ema_step=17, decay=0.95, seed=1337),
    "B_ragged": dict(scene="shaped", start="untrained", max_cascade=0, n_uniform=(1 << 19) + 37, n_nonuniform=(1 << 17) + 5, ema_step=17, decay=0.95, seed=1337),
    # C: four cascades, the cell-order path with random levels and a non-uniform draw behind it (the Trainer's call after step 256 with max_cascade 3, second draw shortened)
    "C": dict(scene="shaped16", start="untrained16", max_cascade=3, n_uniform=1 << 21, n_nonuniform=(1 << 19) + 37, ema_step=5, decay=0.95, seed=1337),
    # step * n passes 2^32: 70000 * (3 * 2^15 + 21) = 6.9e9
    "C_wrap": dict(scene="shaped16", start="untrained16", max_cascade=2, n_uniform=3 * (1 << 15) + 21, n_nonuniform=(1 << 15) + 5, ema_step=70000, decay=0.95, seed=1337),
}
for _n, _c in CASES.items():
    _c.update(oracle_bits=_n in ("A", "B"), min_share=0.99)
# E: parameter blobs in other value regimes, from a grid of zeros.  With the Trainer's start weights every raw density is a few 1e-5, exp() of it rounds to fp16 1.0 and
# every sampled cell receives the SAME thickness, 1.0 * MIN_STEP.  So E_initial_dense (one sample per cell, no untrained cell) gives a grid whose every cell EQUALS its
# mean: no cell lies above the threshold and the bitfield is empty, on the oracle and in the reference's formula alike -- and one ulp of error in the device's mean
# would set all 2^21 bits.  The dense bitfield with the mean in charge is E_initial_untrained: the same call from a grid with untrained blocks, where the mean is the
# thickness times the share of trained cells and every trained cell lies above it.
REGIME_BLOBS = ("initial", "large", "overflow")
INITIAL_SEED = 11
for _name in REGIME_BLOBS:
    CASES["E_" + _name] = dict(scene=_name, start="zeros", max_cascade=0, n_uniform=(1 << 17) + 3, n_nonuniform=0, ema_step=0, decay=0.95, seed=1337,
                               oracle_bits=False, min_share=0.99)
CASES["E_initial_dense"] = dict(scene="initial", start="zeros", max_cascade=0, n_uniform=1 << 21, n_nonuniform=0, ema_step=0, decay=0.95, seed=1337,
                                oracle_bits=False, min_share=0.99)
CASES["E_initial_untrained"] = dict(CASES["E_initial_dense"], start="zeros_untrained")
WORKER_CASES = ("A", "C")   # repeated in sample order (NRS_REFRESH_ORDER=0) by tests/occupancy_worker.py

# F: what Trainer.update_density_grid hands over: (training step, n_uniform, n_nonuniform, k of decay = 0.95^(k / 16), ema_step going in)
TRAINER_SEED = 11
TRAINER_CALLS = ((0, 1 << 21, 0, 16, 0), (16, 1 << 21, 0, 16, 1), (256, 1 << 19, 1 << 19, 240, 2), (272, 1 << 19, 1 << 19, 16, 3))
TRAINER_CALLS_CASCADE3 = ((0, 1 << 23, 0), (256, 1 << 21, 1 << 21))   # max_cascade 3: (training step, n_uniform, n_nonuniform)


def n_samples(case):
    return case["n_uniform"] + case["n_nonuniform"]


def grid_update(case):
    """The _abi.GridUpdate of a case (fresh: both sides get their own copy)."""
    from nerfshop_amd import _abi, runtime
    u = _abi.GridUpdate()
    u.n_uniform_samples, u.n_nonuniform_samples = case["n_uniform"], case["n_nonuniform"]
    u.reset_grid, u.max_cascade, u.decay, u.ema_step = 0, case["max_cascade"], case["decay"], case["ema_step"]
    u.rng_state, u.rng_inc = runtime.rng_seed(case["seed"])
    return u


def copy_update(u):
    from nerfshop_amd import _abi
    v = _abi.GridUpdate()
    for f, _ in _abi.GridUpdate._fields_:
        setattr(v, f, getattr(u, f))
    return v


def untrained_grid(base_grid, seed, share=0.5):
    """base_grid with whole 4 x 4 x 4 blocks (64 consecutive Morton cells) of every cascade set to -1, each block with probability `share`."""
    out = np.array(base_grid, np.float32, copy=True)
    assert out.size == CASCADES * VOL
    hit = np.random.default_rng(seed).random(out.size // 64) < share
    out.reshape(-1, 64)[hit] = -1.0
    return out


class Oracle:
    """The oracle's side of every case, computed once and shared: Oracle(scene_shaped, scene16_shaped) from conftest's Scene objects.  start(name) is a start grid
    (never written to: callers copy), model(name) / params(name) the oracle model and parameter blob of a case's `scene`, run(case name) the oracle's refresh of the
    case from a copy of its start grid: (GridUpdate afterwards, grid, bitfield)."""

    def __init__(self, scene_shaped, scene16_shaped):
        self.scenes = {"shaped": scene_shaped, "shaped16": scene16_shaped}
        self.desc = scene_shaped.desc
        self._starts, self._models, self._runs = {}, {}, {}

    def params(self, name):
        if name in self.scenes:
            return self.scenes[name].params
        self.model(name)
        return self._models[name][0]

    def model(self, name):
        if name in self.scenes:
            return self.scenes[name].oracle_model
        if name not in self._models:
            from oracle import oracle as orc
            p = regime_blob(name, self.desc)
            self._models[name] = (p, orc.Model(self.desc, p, None))
        return self._models[name][1]

    def refresh(self, name, grid, update):
        """One oracle call on `grid` (in place); the scene's own bitfield is put back into its model afterwards (Model.update_density_grid installs the new one)."""
        bits = self.model(name).update_density_grid(grid, update, [])
        if name in self.scenes:
            self.scenes[name].oracle_model.set_bitfield(self.scenes[name].bitfield)
        return bits

    def start(self, name):
        """`untrained`: the oracle's own refresh of the shaped scene (one uniform sample per cell of cascade 0) with untrained blocks.  `untrained16`: the same for the
        aabb_scale-16 scene over all five cascades (2^21 samples at random levels: a fifth of every cascade's cells hold a value), doubled, untrained blocks in all five.
        `zeros_untrained`: nothing but untrained blocks."""
        if name not in self._starts:
            zeros = np.zeros(CASCADES * VOL, np.float32)
            if name == "zeros":
                g = zeros
            elif name == "zeros_untrained":
                g = untrained_grid(zeros, UNTRAINED_SEED)
            else:
                scene, max_cascade = {"untrained": ("shaped", 0), "untrained16": ("shaped16", 4)}[name]
                case = dict(n_uniform=VOL, n_nonuniform=0, max_cascade=max_cascade, decay=0.95, ema_step=0, seed=1337)
                self.refresh(scene, zeros, grid_update(case))
                if name == "untrained16":
                    zeros *= np.float32(2)   # the solid's thickness is 0.009 in this scene: doubled, it lies above 0.01 and the non-uniform draw has cells to find
                g = untrained_grid(zeros, UNTRAINED_SEED)
            g.setflags(write=False)
            self._starts[name] = g
        return self._starts[name]

    def run(self, case_name):
        if case_name not in self._runs:
            case = CASES[case_name]
            grid, u = self.start(case["start"]).copy(), grid_update(case)
            bits = self.refresh(case["scene"], grid, u)
            grid.setflags(write=False)
            self._runs[case_name] = (u, grid, bits)
        return self._runs[case_name]


def regime_blob(name, desc):
    """The parameter blobs of case E (uint16 bits): the Trainer's start rounded to fp16, and tests/value_regimes.py's `large` and `overflow`."""
    import torch
    from nerfshop_amd import synth
    from nerfshop_amd.torch_module import initial_params
    import value_regimes as vr
    n = vr.N_NET + 2 * int(synth.level_table(desc)["offset"][15] + synth.level_table(desc)["count"][15])
    if name == "initial":
        return initial_params(n, INITIAL_SEED).to(torch.float16).numpy().view(np.uint16).copy()
    base = synth.make_params(desc, sigma_raw=synth.default_sigma_raw(1))
    assert base.size == n
    return vr.make_regime(name, desc, base)


def sample_cells(grid_cascade, n, step, thresh):
    """The sampler's cell choice for one draw of n samples with n_cascades == 1, in uint32 arithmetic: (cell [n], tries [n] in 1..10, exhausted [n]).  A sample is
    exhausted when none of its ten cells lies above `thresh`: it keeps the tenth."""
    g = np.asarray(grid_cascade, np.float32)
    assert g.size == VOL
    i = np.arange(n, dtype=np.uint32)
    with np.errstate(over="ignore"):
        base = (i + np.uint32((step * n) & 0xffffffff)) * np.uint32(SAMPLE_MUL) + np.uint32(SAMPLE_ADD)
        cell = np.zeros(n, np.uint32)
        tries = np.zeros(n, np.uint32)
        open_ = np.ones(n, bool)
        for j in range(10):
            idx = (base + np.uint32((j * SAMPLE_STEP) & 0xffffffff)) % np.uint32(VOL)
            cell[open_] = idx[open_]
            tries[open_] = j + 1
            open_ &= ~(g[idx] > thresh)
    return cell, tries, open_


def sequential_mean(grid):
    """The oracle's order (orc_density_grid_to_bitfield): term after term in float64, rounded to float32 at the end."""
    terms = (np.maximum(np.asarray(grid[:VOL], np.float32), np.float32(0)) / np.float32(VOL)).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.float32(np.cumsum(terms)[-1])   # (cumsum is a running sum: no pairwise blocking)


def tree_mean(grid):
    """The device's order (grid_mean_partial_kernel / grid_mean_final_kernel): block b owns cells [8192 b, 8192 (b + 1)); its thread t adds cells t, t + 256, ... one
    after the other; the 256 partial sums are halved (part[t] += part[t + s], s = 128 .. 1); the 256 block sums are halved the same way; float32 at the end."""
    terms = (np.maximum(np.asarray(grid[:VOL], np.float32), np.float32(0)) / np.float32(VOL)).astype(np.float64).reshape(256, 32, 256)
    with np.errstate(over="ignore", invalid="ignore"):
        part = np.zeros((256, 256), np.float64)
        for k in range(32):
            part = part + terms[:, k, :]
        s = 128
        while s:
            part = part[:, :s] + part[:, s:2 * s]
            s >>= 1
        blocks = part[:, 0]
        s = 128
        while s:
            blocks = blocks[:s] + blocks[s:2 * s]
            s >>= 1
        return np.float32(blocks[0])


def threshold(grid):
    return min(np.float32(0.01), sequential_mean(grid))


def near_threshold_cells(grid, rel=1.5e-2):
    """Cells of cascade 0 within `rel` of the bitfield's threshold: where test_gpu_grid_refresh._compare lets a bit of the device differ from the oracle's."""
    t = threshold(grid)
    return int((np.abs(grid[:VOL] - t) <= np.float32(rel) * t).sum())
