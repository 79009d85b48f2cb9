"""Short rays, saturated alpha and min_transmittance at its edges.

Every other scene of the suite has default_sigma_raw's opacity (alpha ~ 0.14 per sample, ~26-33 samples per ray).  A trained snapshot lives where rays end
within a few samples (VERDICT weak #4), and that is where lane teams end a ray at lane k < TEAM of a round (nrs_render.cuh: the later samples of the round
must be dropped).  Here the network's constant density channel is set for an opacity per sample of (synth.sigma_for_alpha)

  0.005   rays leave the box unsaturated (n* ~ 900 samples)        0.5    n* = ln(min_transmittance) / ln(1 - alpha) = 6.6 samples
  0.84    n* = 2.5                                                  0.954  n* = 1.5
  1.0     exactly 1.0f: 1 - __expf(-sigma dt) rounds to 1 for every sample (sigma dt = 40 e), a ray ends at its first sample

with the tests' min_transmittance of 0.01 (synth.render_params).  Round values (0.9: n* = 2.0, 0.99: n* = 1.0) are avoided: there the test
`accumulated alpha > 1 - min_transmittance` of most pixels is decided by the last ulp, and the sample-count bar would fail for a reason that says nothing
about the kernel.  Each scene is first shown to be in its regime on the oracle's side; the GPU frame is then held to the unchanged bars of
tests/test_gpu_parity.py (_compare_frames) with one lane per ray, and every schedule must give its bits.  Also min_transmittance 0 and 1 (its valid
edges) and max_march_steps 1 / 2 / 3 on short rays.  The oracle is pinned to the reference's own code in this regime by tests/test_ref_pin.py (the
lego_a084 / lego_a1 / lego_a05_mt* cases)."""
import math

import numpy as np
import pytest

from test_gpu_route_matrix import Rigs, route_on, render_schedules, assert_same

pytestmark = pytest.mark.gpu

ALPHAS = (0.005, 0.5, 0.84, 0.954, 1.0)
SIZE = (160, 96)
# (route of tests/test_gpu_route_matrix.py, rig): cage, cage + membrane, cage + affine, numerics + cage, aabb 16 (cone stepping: its own dt), and the
# shaped scene with varied opacity (geometry in the network, density_noise 1.5)
CASES = [("R2_cage", "lego"), ("R3_membrane_t0", "lego"), ("R5_cage_affine", "lego"), ("R7_num11_cage", "lego"), ("R11_gate_cage", "aabb16"),
         ("R2_cage", "shaped")]


@pytest.fixture(scope="module")
def alpha_rigs(built):
    from conftest import GpuRig, Scene
    rigs = Rigs(lego=GpuRig(Scene(aabb_scale=1, with_edit=True, lattice_n=6)), aabb16=GpuRig(Scene(aabb_scale=16, with_edit=True, lattice_n=5)),
                shaped=GpuRig(Scene(aabb_scale=1, with_edit=True, lattice_n=6, shaped=True)))
    rigs._alpha = {}
    return rigs


def set_alpha(rigs, key, alpha):
    """the rig's network (both sides) with the opacity `alpha` per sample (ref_pin_cases.alpha_scene)"""
    import ref_pin_cases as cases
    rig = rigs.get(key)
    if rigs._alpha.get(key) != alpha:
        cases.alpha_scene(rig.scene, alpha, shaped=(key == "shaped"), density_noise=1.5 if key == "shaped" else 0.25)
        rig.net.set_params(rig.scene.params)
        rigs._alpha[key] = alpha
    return rig


def n_star(alpha, min_transmittance=0.01):
    return math.inf if alpha <= 0 else (1 if alpha >= 1 else math.log(min_transmittance) / math.log1p(-alpha))


def assert_regime(key, alpha, ref):
    """the oracle's frame is in the regime the case is for (measured at 160x96: lego / aabb 16 -- median samples per hit pixel 111 / 27, 7 / 6, 3 / 3,
    2 / 2, 1 / 1 for the five opacities, >= 97 % of the hit pixels saturated from 0.5 up, 99.9 % with one sample at 1.0; the shaped scene is transparent
    outside its solid: 24 % of its hit pixels end at the first sample at 1.0, the rest cross empty cells first)"""
    frame, _, steps, _ = ref
    hit = steps > 0
    s, a = steps[hit], frame[..., 3][hit]
    assert hit.sum() > 1000
    if alpha < 0.01:
        # (>= 99.9 % without the membrane correction, whose outside density saturates 4 % of the rays of the membrane route)
        assert (a < 0.9).mean() >= 0.9 and np.median(s) >= 20, ("rays should leave the box unsaturated", (a < 0.9).mean(), np.median(s))
        return
    saturated = (a >= 0.99).mean()
    if key == "shaped":
        assert saturated >= 0.85, saturated
        if alpha == 1.0:
            assert (s == 1).mean() >= 0.2, (s == 1).mean()
        return
    assert saturated >= 0.9, saturated
    assert np.median(s) <= math.ceil(n_star(alpha)), (alpha, np.median(s))
    if alpha == 1.0:
        assert (s == 1).mean() >= 0.9, (s == 1).mean()


def _check(rig, ref_ops, p, ref=None, flat_weights=False):
    """one lane per ray against the oracle at tests/test_gpu_parity.py's bars, every schedule bit-equal to it.

    flat_weights (rays that never saturate, alpha 0.005): the depth buffer holds the position of the sample of largest weight T_i alpha_i
    (tn: payload.max_weight).  With ~100 samples of alpha 0.005 the weights fall by 0.5 % per sample while the density noise moves alpha by up to
    +-25 %, so the largest and the runner-up are often within a few fp16 ulps of the network output (the network bar: <= 4 ulps = 0.4 %) and
    which one is larger is decided by that last ulp: the depth of such a pixel jumps along the ray in either implementation.  There the depth bar
    is stated per ray -- finite, inside the box segment of the oracle's samples (between the nearest and the farthest depth of a hit pixel) -- and
    the 2e-3 bar holds for >= 90 % of the hit pixels; the frame and sample-count bars are unchanged."""
    from test_gpu_parity import _compare_frames
    out = render_schedules(rig, p)
    frame, depth, steps, st, _ = out[1]
    ref = ref or rig.scene.oracle_model.render(p, ref_ops)
    assert st.n_rays_alive == ref[3].n_alive0
    if flat_weights:
        d = np.abs(frame - ref[0])
        assert d.max() < 6e-3 and d.mean() < 2e-4, (d.max(), d.mean())
        ds = np.abs(steps.astype(np.int64) - ref[2].astype(np.int64))
        assert ds.max() <= 1 and (ds == 0).mean() >= 0.998, (ds.max(), (ds == 0).mean())
        hit = (ref[0][..., 3] > 0.2) & (frame[..., 3] > 0.2) & (ds == 0)
        near = np.abs(depth[hit] - ref[1][hit]) <= 2e-3
        print(f"flat weights: depth within 2e-3 for {near.mean():.4f} of {hit.sum()} hit pixels")
        lo, hi = ref[1][ref[2] > 0].min(), ref[1][ref[2] > 0].max()
        assert np.isfinite(depth[hit]).all() and (depth[hit] >= lo - 2e-3).all() and (depth[hit] <= hi + 2e-3).all()
        assert near.mean() >= 0.9, near.mean()
        miss = (ref[0][..., 3] == 0) & (frame[..., 3] == 0)
        assert (depth[miss] == 1e10).all() and (ref[1][miss] == 1e10).all()
    else:
        _compare_frames(frame, depth, steps, ref[0], ref[1], ref[2])
    assert_same(out, f"{p.min_transmittance} {p.max_march_steps}")
    return ref, st


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("route,key", CASES, ids=[f"{r}-{k}" for r, k in CASES])
def test_opacity(alpha_rigs, route, key, alpha):
    set_alpha(alpha_rigs, key, alpha)
    with route_on(alpha_rigs, route, size=SIZE, rig_key=key) as (rig, ref_ops, p):
        ref = rig.scene.oracle_model.render(p, ref_ops)
        assert_regime(key, alpha, ref)
        _check(rig, ref_ops, p, ref, flat_weights=alpha < 0.01)


@pytest.mark.parametrize("alpha", [0.5, 1.0])
@pytest.mark.parametrize("min_transmittance", [0.0, 1.0])
def test_min_transmittance_edges(alpha_rigs, alpha, min_transmittance):
    """0: no ray saturates (transmittance stays > 0 until the box exit or max_march_steps; 128x72 -- rays of several hundred samples);
    1: a ray ends at its first sample with alpha > 0 (`accumulated alpha > 0`)"""
    set_alpha(alpha_rigs, "lego", alpha)
    size = (128, 72) if min_transmittance == 0.0 else SIZE
    with route_on(alpha_rigs, "R2_cage", size=size) as (rig, ref_ops, p):
        p.min_transmittance = min_transmittance
        ref, st = _check(rig, ref_ops, p)
        s = ref[2][ref[2] > 0]
        if min_transmittance == 1.0:
            assert (s == 1).mean() >= 0.99, (s == 1).mean()
        elif alpha < 1.0:
            assert np.median(s) > 50, np.median(s)  # far beyond n* = 6.6 of min_transmittance 0.01


@pytest.mark.parametrize("alpha", [0.84, 1.0])
@pytest.mark.parametrize("cap", [1, 2, 3])
def test_step_cap_on_short_rays(alpha_rigs, alpha, cap):
    """max_march_steps 1 / 2 / 3 where rays end after ~2.5 samples (0.84) or one (1.0): the cap and the saturation decide in the same rounds, and
    every schedule gives the bits of one lane per ray.

    Not against the oracle: the reference's bound is on its compaction loop, `i += n_steps_between_compaction` while i < MARCH_ITER (tn:2812-2835;
    oracle/nrs_oracle.cpp and the reference's own code agree), so a small cap cuts a ray after a number of samples that depends on how many rays of the
    whole frame are alive (cap 1: nothing is traced at all).  The kernels cap each ray's own sample count (render_body: n_steps >= max_steps) -- the
    same frames at the default MARCH_ITER, where no ray of these scenes comes near the bound, different ones where a small cap binds."""
    set_alpha(alpha_rigs, "lego", alpha)
    with route_on(alpha_rigs, "R2_cage", size=SIZE) as (rig, ref_ops, p):
        p.max_march_steps = cap
        out = render_schedules(rig, p)
        assert_same(out, f"max_march_steps {cap}")
        steps, st = out[1][2], out[1][3]
        assert steps.max() <= cap and st.n_samples > 1000
