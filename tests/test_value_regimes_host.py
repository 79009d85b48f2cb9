"""tests/value_regimes.py without a GPU: the float64 interval reference against the oracle's own activations (the oracle standing in for the device), the
regimes' preconditions, and the two mutations the GPU tests must notice (a table with its subnormals flushed, two weight rows swapped in the reference)."""
import numpy as np
import pytest

import value_regimes as vr

N = 512 + 3


@pytest.fixture(scope="module")
def models(built):
    from nerfshop_amd import synth
    from oracle import oracle as orc
    desc = synth.model_desc(1)
    base = synth.make_params(desc, sigma_raw=synth.default_sigma_raw(1))
    cache = {}

    def get(name):
        if name not in cache:
            p = base if name == "default" else vr.make_regime(name, desc, base)
            cache[name] = (desc, p, orc.Model(desc, p, None))
        return cache[name]
    return get


@pytest.mark.parametrize("acc16", [False, True])
@pytest.mark.parametrize("name", ["default", "tcnn_init", "subnormal", "amplified", "wide", "large"])
def test_the_oracle_lies_in_the_reference_interval(models, name, acc16):
    desc, p, model = models(name)
    c = vr.regime_coords(name, desc, N, 5) if name != "default" else vr.coords(N, 5)
    model.set_numerics(int(acc16), int(acc16))
    try:
        acts = vr.oracle_activations(model, c)
    finally:
        model.set_numerics(0, 0)
    report, failures = vr.check_chain(acts, p, acc16=acc16)
    assert not failures, failures
    assert all(r["inside"] == 1.0 for r in report.values())
    if not acc16:   # the interval is tight: one fp16 value for most units, never more than two adjacent ones
        assert all(r["single_value"] > 0.6 for r in report.values()), report


def test_regimes_are_in_their_regimes(models):
    desc, p, model = models("tcnn_init")
    table = vr.weights(p)["table"]
    assert 0.55 < vr.is_subnormal(table[:1 << 22]).mean() < 0.67 and np.abs(table[1 << 20:1 << 22].astype(np.float32)).max() <= 1.001e-4
    acts = vr.oracle_activations(model, vr.regime_coords("tcnn_init", desc, N, 5))
    assert vr.is_subnormal(acts["layer0"]).mean() > 0.9
    desc, p, model = models("subnormal")
    acts = vr.oracle_activations(model, vr.regime_coords("subnormal", desc, N, 5))
    assert vr.is_subnormal(acts["layer0"]).mean() > 0.9 and vr.is_subnormal(acts["layer1"]).mean() > 0.3 and vr.is_subnormal(acts["layer2"][:, 1:16]).mean() > 0.9
    desc, p, model = models("overflow")
    acts = vr.oracle_activations(model, vr.regime_coords("overflow", desc, 2048 + 3, 5))
    assert (vr.value_class(acts["layer1"]) == 1).sum() >= 1 and (vr.value_class(acts["layer2"]) == 2).sum() >= 1
    report, failures = vr.check_chain(acts, p)   # +-inf and NaN follow IEEE in the reference as in the oracle
    assert not failures, failures
    desc, p, model = models("zero")
    acts = vr.oracle_activations(model, vr.regime_coords("zero", desc, N, 5))
    assert not acts["layer3"].any() and not acts["layer4"].any() and (acts["outputs"][:, 3] == vr.weights(p)["dw2"][0, 0]).all()
    assert (acts["outputs"][:, :3] == 0).all()


def test_a_flushed_table_leaves_the_interval(models):
    """Mutation: the oracle on a table whose subnormals are flushed, checked against the TRUE blob's reference, as a flushing device would be."""
    from oracle import oracle as orc
    desc, p, model = models("amplified")
    c = vr.regime_coords("amplified", desc, N, 5)
    flushed = orc.Model(desc, vr.flush_subnormals(p), None)
    acts = vr.oracle_activations(flushed, c)
    true_layer0 = model.hashgrid_encode(c)
    assert (acts["layer0"].astype(np.float16).view(np.uint16) != true_layer0).mean() > 0.5   # the bit-exact layer-0 check sees it
    # ... and a device that flushed only inside the first matrix product (true features in, flushed features used) leaves layer 1's interval
    acts_true = dict(acts, layer0=true_layer0.view(np.float16).astype(np.float32))
    report, failures = vr.check_chain(acts_true, p)
    assert failures and report["layer1"]["inside"] < 0.6, report["layer1"]


def test_swapped_weight_rows_leave_the_interval(models):
    """Mutation of the reference side: two rows of one matrix swapped in the blob the reference reads."""
    desc, p, model = models("tcnn_init")
    acts = vr.oracle_activations(model, vr.regime_coords("tcnn_init", desc, N, 5))
    for key, rows in (("dw1", (5, 6)), ("dw2", (2, 9)), ("rw1", (0, 63)), ("rw2", (10, 11)), ("rw3", (0, 1))):
        q = p.copy()
        w = vr.weights(q)[key]
        w[list(rows)] = w[list(rows)[::-1]].copy()
        report, failures = vr.check_chain(acts, q)
        assert len(failures) == 1 and failures[0].startswith({"dw1": "layer1", "dw2": "layer2", "rw1": "layer3", "rw2": "layer4", "rw3": "outputs"}[key]), (key, failures)


def test_interval_arithmetic():
    """layer_interval on hand-made cases: exact sums give one value, the bound scales with the magnitudes, inf and NaN follow IEEE, ReLU clamps both ends."""
    W = np.zeros((2, 32))
    W[0, :2] = (1.0, 2.0 ** -10)
    W[1, :2] = (-1.0, 1.0)
    X = np.zeros((3, 32))
    X[0, :2] = (2.0 ** -24, 2.0 ** -14)       # 2^-24 + 2^-24: exactly 2^-23, a subnormal
    X[1, :2] = (65504.0, 65504.0)
    X[2, :2] = (np.inf, 1.0)
    lo, hi, s, B = vr.layer_interval(X, W, relu=False)
    assert lo[0, 0] == hi[0, 0] == 2.0 ** -23 and s[0, 0] == 2.0 ** -23 and 0 < B[0, 0] < 2.0 ** -40
    assert lo[1, 0] == hi[1, 0] == np.inf                                  # 65504 + 63.97 rounds to inf in fp16 (>= 65520)
    assert s[1, 1] == 0 and lo[1, 1] == -hi[1, 1] and 0.4 < hi[1, 1] < 0.5   # cancellation: the bound follows the magnitudes of the terms (2 x 31 x 2^-24 x 131008), not of the sum
    assert lo[2, 0] == hi[2, 0] == np.inf and lo[2, 1] == hi[2, 1] == -np.inf
    lo, hi, _, _ = vr.layer_interval(X, W, relu=True)
    assert lo[2, 1] == hi[2, 1] == 0 and lo[0, 0] == 2.0 ** -23
    assert vr.inside(np.array([[np.nan]]), np.array([[np.nan]]), np.array([[np.nan]])).all() and not vr.inside(np.array([[0.0]]), np.array([[np.nan]]), np.array([[np.nan]])).any()
