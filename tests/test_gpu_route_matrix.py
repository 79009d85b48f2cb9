"""Every render route x every schedule x whole image and tiles.

plan_route (nrs_route.h) picks one row of the table of ~40 render_kernel instantiations (TEAM, POISSON, AFFINE, NUM, EXTRA) and nrs_render_nerf sizes the
launch from that row (a.team: 0 = automatic schedule, 1 / 2 / 4 = fixed lanes per ray; the packet / tile geometry).  Were the packets sized for another TEAM
than the kernel's, packet_pixel would lay out pixels with another packet shape than the launch was sized for: whole images come out right with wasted
packets, a tiled launch writes past its compact buffers.  The last guard (nrs_render.hip check_route) refuses such a launch, and tests/test_route_plan_host.py
asks the same of every plan without a GPU; these tests render every route the library has --

  R1 no edit            R2 cage                 R3 cage + membrane (target 0 / 1)   R4 AffineDuplication (hide_original)   R5 cage + affine
  R6 membrane + affine  R7 numerics (1,1) + cage R8 numerics (1,0) / (0,1)         R9 numerics + cage + affine           R10 3-layer rgb (DEEP) + cage
  R11 aabb 16 (GATE)    R12 Depth over cage     R13 Normals over cage              R14 Depth over membrane + affine
  and, so that every instantiation reachable without development knobs is rendered (test_every_reachable_instantiation_is_rendered):
  R15 numerics + membrane, R16 / R17 numerics + Depth / Normals, R18 DEEP + Normals, R19 DEEP + numerics, R20 DEEP + numerics + Normals

-- (a) with one lane per ray against the oracle at the existing bars (tests/test_gpu_parity.py _compare_frames for Shade, tests/test_gpu_modes.py _compare
for the modes; the 3-layer network: tests/test_gpu_architectures.py's bar for it), (b) under all eight schedules bit for bit equal to (a) at an odd
whole-image size, (c) on tiles of 32 and 64 pixels, two (tile_first, tile_stride) deals each, under the same schedules: every owned pixel of frame, depth
and step counts bit-equal to the pixel of (a) it stands for (nrs.h: pixel (tx, ty) of the k-th owned tile at ((k * T + ty) * T + tx)).

Every buffer is guarded: a tail of at least as many tiles as are owned (whole images: extra rows) filled with a sentinel bit pattern, and the pixels of edge
tiles that lie outside the image hold it too (packet_pixel returns false there: nothing is written) -- after each render both must be bit-unchanged."""
import contextlib
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

AO, SHADE, NORMALS, POSITIONS, DEPTH = range(5)
SCHEDULES = (1, 2, 4, -1, -2, -3, -4, 0)
WHOLE = (173, 131)
TILINGS = ((32, 5, 8), (32, 1, 3), (64, 5, 8), (64, 1, 3))  # (tile size, tile_first, tile_stride)
SENTINEL = 0x7FC0FFEE  # a quiet-NaN bit pattern: no float the renderer writes has it
EXTRA_ROWS = 9

ROUTES = {
    "R1_noedit": dict(),
    "R2_cage": dict(edits=("cage",)),
    "R3_membrane_t0": dict(edits=("membrane",)),
    "R3_membrane_t1": dict(edits=("membrane",), fields={"poisson_target": 1}),
    "R4_affine": dict(edits=("affine_hide",)),
    "R5_cage_affine": dict(edits=("cage", "affine")),
    "R6_membrane_affine": dict(edits=("membrane", "affine")),
    "R7_num11_cage": dict(edits=("cage",), numerics=(1, 1)),
    "R8_num10": dict(numerics=(1, 0)),
    "R8_num01": dict(numerics=(0, 1)),
    "R9_num11_cage_affine": dict(edits=("cage", "affine"), numerics=(1, 1)),
    "R10_deep_cage": dict(rig="rgb3", edits=("cage",)),
    "R11_gate_cage": dict(rig="aabb16", edits=("cage",)),
    "R12_depth_cage": dict(edits=("cage",), fields={"render_mode": DEPTH, "depth_scale": 0.7}),
    "R13_normals_cage": dict(edits=("cage",), fields={"render_mode": NORMALS}),
    "R14_depth_membrane_affine": dict(edits=("membrane", "affine"), fields={"render_mode": DEPTH, "depth_scale": 0.7}),
    "R15_num11_membrane": dict(edits=("membrane",), numerics=(1, 1)),
    "R16_num11_depth_cage": dict(edits=("cage",), numerics=(1, 1), fields={"render_mode": DEPTH, "depth_scale": 0.7}),
    "R17_num11_normals_cage": dict(edits=("cage",), numerics=(1, 1), fields={"render_mode": NORMALS}),
    "R18_deep_normals_cage": dict(rig="rgb3", edits=("cage",), fields={"render_mode": NORMALS}),
    "R19_deep_num11_cage": dict(rig="rgb3", edits=("cage",), numerics=(1, 1)),
    "R20_deep_num11_normals": dict(rig="rgb3", edits=("cage",), numerics=(1, 1), fields={"render_mode": NORMALS}),
}

# Every instantiation plan_route (nrs_route.h) can reach without development knobs, as its NRS_KERNEL_LOG line names it.  Entries on the 128-register
# entry point (render_kernel_c128) fall back to their __launch_bounds__(512, 4) twin render_kernel<8, 4, ...> when the register allocator went past 128
# VGPRs: either name is accepted for those, and the test reports which one ran.
C128 = "render_kernel_c128<8, prof {p}, poisson {q}, affine {a}, team {t}, num {n}, extra {x}>"
CFG = "render_kernel<{w}, {o}, prof {p}, poisson {q}, affine {a}, team {t}, num {n}, extra {x}>"
R = -1  # kNumRuntime (nrs_route.h): the run-time numerics twin, printed as its value
REACHABLE_C128 = [  # (poisson, affine, team, num, extra)
    (0, 0, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 2, 0, 0), (0, 0, 4, 0, 0),    # the default kernel: automatic schedule, fixed 1 / 2 / 4 lanes per ray
    (0, 1, 0, 0, 0),                                                       # AffineDuplication, automatic schedule
    (0, 0, 0, 1, 0), (0, 0, 0, 2, 0), (0, 0, 0, 3, 0),                     # compile-time numerics, automatic schedule
    (0, 0, 0, 0, 6),                                                       # GATE (cone stepping)
    (0, 0, 1, 0, 1),                                                       # lean EXTRA (a mode over cage edits)
]
REACHABLE_CFG = [  # (waves, occ, poisson, affine, team, num, extra)
    (8, 4, 0, 1, 1, 0, 0),                                                 # AffineDuplication, one lane per ray
    (8, 4, 1, 0, 0, 0, 0),                                                 # membrane correction, automatic schedule
    (12, 3, 1, 1, 1, 0, 0),                                                # the Shade catch-all: membrane + affine, membrane with a forced schedule
    (8, 3, 0, 0, 1, R, 0), (8, 3, 0, 0, 2, R, 0), (8, 3, 0, 0, 4, R, 0),    # run-time numerics, fixed lanes per ray
    (8, 3, 0, 1, 1, R, 0), (12, 3, 1, 1, 1, R, 0),                         # run-time numerics with AffineDuplication / the membrane correction
    (8, 4, 0, 0, 0, 0, 5),                                                 # DEEP, automatic schedule
    (12, 3, 1, 1, 1, 0, 1), (12, 3, 1, 1, 1, R, 1),                        # EXTRA catch-all
    (12, 3, 1, 1, 1, 0, 2), (12, 3, 1, 1, 1, R, 2),                        # INTRO (Normals / EncodingVis)
    (12, 3, 1, 1, 1, 0, 3), (12, 3, 1, 1, 1, R, 3),                        # DEEP EXTRA
    (12, 3, 1, 1, 1, 0, 4), (12, 3, 1, 1, 1, R, 4),                        # DEEP INTRO
]
# reachable only through development knobs (NRS_DEV_KNOBS=1), not rendered here:
#   NRS_DEBUG bit 2 (wave log): render_kernel<8, 4, prof 1, ..., team 0 | 1, num 0, extra 0>
#   NRS_RENDER_CFG=84: render_kernel<8, 4, prof 0, ...> for the default kernel's schedules and AffineDuplication team 0 (the c128 entries' twins)
#   NRS_RENDER_CFG=42: render_kernel<4, 2, prof 0, poisson 0, affine 0, team 1, num 0, extra 0>
#   NRS_RENDER_CFG=124: render_kernel<12, 3, prof 0, poisson 1, affine 0, team 0, num 0, extra 0>
#   NRS_DEBUG bit 2 / NRS_RENDER_CFG with numerics on the automatic schedule: render_kernel<8, 3, prof 0, poisson 0, affine 0, team 0, num -1, extra 0>


def expected_instantiations():
    """-> [(accepted names, ...)] one tuple per reachable instantiation"""
    out = []
    for (q, a, t, n, x) in REACHABLE_C128:
        out.append((C128.format(p=0, q=q, a=a, t=t, n=n, x=x), CFG.format(w=8, o=4, p=0, q=q, a=a, t=t, n=n, x=x)))
    for (w, o, q, a, t, n, x) in REACHABLE_CFG:
        out.append((CFG.format(w=w, o=o, p=0, q=q, a=a, t=t, n=n, x=x),))
    return out


# ---- rigs and routes -------------------------------------------------------------------------------------------------------------------------------
class Rigs:
    """GpuRig per scene, built on demand: lego (conftest's), aabb 16 (cone stepping), the 3-layer rgb network (tests/test_gpu_architectures.py's)"""

    def __init__(self, **given):
        self._r = dict(given)
        self._bits = {}

    def get(self, key):
        if key not in self._r:
            from conftest import GpuRig, Scene
            if key == "lego":
                self._r[key] = GpuRig(Scene(aabb_scale=1, with_edit=True, lattice_n=6))
            elif key == "aabb16":
                self._r[key] = GpuRig(Scene(aabb_scale=16, with_edit=True, lattice_n=5))
            elif key == "rgb3":
                self._r[key] = GpuRig(Scene(aabb_scale=1, with_edit=True, lattice_n=6, shaped=True, rgb_hidden_layers=3))
            else:
                raise KeyError(key)
        return self._r[key]

    def bitfield(self, key, kinds, ref_ops):
        """occupancy seen through the route's operators (cached: the deformed grid is a CPU walk)"""
        rig = self.get(key)
        if not ref_ops:
            return rig.scene.bitfield
        if not any(k.startswith("affine") for k in kinds):
            return rig.scene.edited_bitfield  # (the membrane terms do not move anything)
        if (key, kinds) not in self._bits:
            from test_gpu_affine import _edited_bitfield
            self._bits[(key, kinds)] = _edited_bitfield(rig.scene, ref_ops)
        return self._bits[(key, kinds)]


@contextlib.contextmanager
def route_on(rigs, route, size=WHOLE, rig_key=None):
    """installs a route on its rig (operators, occupancy, numerics on both sides); yields (rig, oracle operators, render params)"""
    from oracle import oracle as orc
    spec = ROUTES[route]
    key = rig_key or spec.get("rig", "lego")
    rig = rigs.get(key)
    scene = rig.scene
    kinds = spec.get("edits", ())
    dev_ops, ref_ops, owned = [], [], []
    try:
        for kind in kinds:
            if kind == "cage":
                dev_ops.append(rig.op)
                ref_ops.append(scene.oracle_edit)
            elif kind == "membrane":
                edit = scene.edit.with_membrane(residual_amplitude=0.8)
                op = rig.rt.CageDeformation(rig.ctx, scene.desc, edit)
                owned.append(op)
                dev_ops.append(op)
                ref_ops.append(orc.Edit(scene.desc, edit.tet_mesh_struct(), keepalive=edit))
            else:
                aff = scene.synth.make_affine_edit(hide_original=(kind == "affine_hide"))
                dev = rig.rt.AffineDuplication(rig.ctx, scene.desc, aff)
                owned.append(dev)
                dev_ops.append(dev)
                ref_ops.append(scene.orc.AffineEdit(scene.desc, aff))
        bits = rigs.bitfield(key, kinds, ref_ops)
        rig.testbed.edit_operators = dev_ops
        rig.net.set_density_bitfield(bits)
        scene.oracle_model.set_bitfield(bits)
        num = spec.get("numerics", (0, 0))
        rig.net.set_numerics(*num)
        scene.oracle_model.set_numerics(*num)
        p = scene.params_for(size[0], size[1], 40.0 if key == "aabb16" else 60.0, apply_operators=bool(kinds))
        for k, v in spec.get("fields", {}).items():
            setattr(p, k, v)
        yield rig, ref_ops, p
    finally:
        rig.ctx.set_lane_teams(0)
        rig.testbed.edit_operators = []
        rig.net.set_numerics(0, 0)
        scene.oracle_model.set_numerics(0, 0)
        rig.net.set_density_bitfield(scene.bitfield)
        scene.oracle_model.set_bitfield(scene.bitfield)
        for op in owned:
            op.close()


# ---- guarded buffers -------------------------------------------------------------------------------------------------------------------------------
def _with(p, **fields):
    q = type(p)()
    C.pointer(q)[0] = p
    for k, v in fields.items():
        setattr(q, k, v)
    return q


def owned_mask(p):
    """-> (owned tiles, mask [owned, T, T] of the pixels that lie inside the image, [(k, x0, y0, w, h)] per owned tile)"""
    from nerfshop_amd import _abi
    lib = _abi.load()
    W, H, T = p.resolution[0], p.resolution[1], p.tile_size
    owned = lib.nrs_render_owned_tiles(C.byref(p))
    pitch = lib.nrs_render_tile_pitch(C.byref(p))
    assert pitch == (((W + T - 1) // T) | 1)
    mask = np.zeros((owned, T, T), bool)
    places = []
    stride = p.tile_stride or 1
    for k in range(owned):
        t = p.tile_first + k * stride
        tx, ty = t % pitch, t // pitch
        w, h = max(0, min(T, W - tx * T)), max(0, min(T, H - ty * T))
        mask[k, :h, :w] = True
        places.append((k, tx * T, ty * T, w, h))
    return owned, mask, places


def guarded_render(rig, p):
    """renders into frame / depth / steps buffers with a sentinel-filled tail (whole images: EXTRA_ROWS rows; tiles: as many tiles again as are owned,
    plus one) and sentinel-filled pixels outside the image; asserts both are untouched.  -> (frame, depth, steps, stats) of the leading part
    ([H, W, ...] or [owned, T, T, ...]), and for tiles the mask of the pixels inside the image"""
    torch = rig.torch
    W, H, T = p.resolution[0], p.resolution[1], p.tile_size
    if T == 0:
        lead = (H, W)
        inside = np.ones(lead, bool)
        full = (H + EXTRA_ROWS, W)
    else:
        owned, inside, _ = owned_mask(p)
        lead = (owned, T, T)
        full = (2 * owned + 1, T, T)
    n_lead = int(np.prod(lead))
    bufs = []
    for ch in (4, 1, 1):
        host = np.full(full + ((ch,) if ch > 1 else ()), SENTINEL, np.uint32)
        head = host[:lead[0]]
        head[inside] = 0  # the caller clears the frame (the renderer composites over it); depth / steps are written for every pixel inside the image
        bufs.append(torch.from_numpy(host.view(np.int32)).to("cuda:0"))
    frame, depth, steps = bufs
    stats = rig.testbed.render_with_params(rig.net, p, frame[:lead[0]].view(torch.float32), depth[:lead[0]].view(torch.float32), steps[:lead[0]], None,
                                           want_stats=True)
    torch.cuda.synchronize()
    out = []
    for b, name in zip(bufs, ("frame", "depth", "steps")):
        h = b.cpu().numpy().view(np.uint32)
        tail = h[lead[0]:]
        assert (tail == SENTINEL).all(), f"{name}: {int((tail != SENTINEL).sum())} words written past the end of the buffer"
        outside = h[:lead[0]][~inside]
        assert (outside == SENTINEL).all(), f"{name}: {int((outside != SENTINEL).sum())} words written to pixels outside the image"
        out.append(h[:lead[0]])
    assert n_lead > 0
    return out[0].view(np.float32), out[1].view(np.float32), out[2], stats, inside


def _stats(st):
    return (st.n_samples, st.n_rays_alive, st.n_rays_hit)


def render_schedules(rig, p):
    out = {}
    try:
        for team in SCHEDULES:
            rig.ctx.set_lane_teams(team)
            out[team] = guarded_render(rig, p)
    finally:
        rig.ctx.set_lane_teams(0)
    return out


def assert_same(out, what):
    ref = out[1]
    for team, (frame, depth, steps, st, _) in out.items():
        assert np.array_equal(frame.view(np.uint32), ref[0].view(np.uint32)), f"{what}: frame differs with schedule {team}"
        assert np.array_equal(depth.view(np.uint32), ref[1].view(np.uint32)), f"{what}: depth differs with schedule {team}"
        assert np.array_equal(steps, ref[2]), f"{what}: step counts differ with schedule {team}"
        assert _stats(st) == _stats(ref[3]), (what, team, _stats(st), _stats(ref[3]))


def assert_tiles_match_whole(tiles, whole, p, what):
    frame, depth, steps = whole[0], whole[1], whole[2]
    _, _, places = owned_mask(p)
    n_px = 0
    for k, x0, y0, w, h in places:
        for got, ref, name in ((tiles[0], frame, "frame"), (tiles[1], depth, "depth"), (tiles[2], steps, "steps")):
            a = np.ascontiguousarray(got[k, :h, :w]).view(np.uint32)
            b = np.ascontiguousarray(ref[y0:y0 + h, x0:x0 + w]).view(np.uint32)
            assert np.array_equal(a, b), f"{what}: {name} of owned tile {k} at ({x0}, {y0}) differs from the whole image in {int((a != b).sum())} words"
        n_px += w * h
    return n_px


def render_route(rigs, route, oracle=True):
    """(a), (b), (c) for one route"""
    from test_gpu_modes import _compare
    from test_gpu_parity import _compare_frames
    with route_on(rigs, route) as (rig, ref_ops, p):
        whole = render_schedules(rig, p)
        frame, depth, steps, st, _ = whole[1]
        if oracle:
            ref = rig.scene.oracle_model.render(p, ref_ops)
            assert ref[3].n_hit > 1000 and st.n_rays_alive == ref[3].n_alive0, (route, ref[3].n_hit, st.n_rays_alive, ref[3].n_alive0)
            if ROUTES[route].get("rig") == "rgb3" and p.render_mode == SHADE:
                # tests/test_gpu_architectures.py's bar for this network: a ray whose last sample sits on the saturation threshold may stop one sample apart
                d = np.abs(frame - ref[0])
                ds = np.abs(steps.astype(np.int64) - ref[2].astype(np.int64))
                assert d.max() < 1.5e-2 and (d.max(axis=-1) > 6e-3).sum() <= 3 and d.mean() < 2e-4, (route, d.max(), d.mean())
                assert ds.max() <= 1 and (ds == 0).mean() >= 0.998
            elif p.render_mode == SHADE:
                _compare_frames(frame, depth, steps, ref[0], ref[1], ref[2])
            else:
                _compare((frame, depth, steps, st), ref)
        assert_same(whole, f"{route} whole image")
        n_tiled = 0
        for T, first, stride in TILINGS:
            q = _with(p, tile_size=T, tile_first=first, tile_stride=stride)
            tiled = render_schedules(rig, q)
            for team, out in tiled.items():
                n_tiled += assert_tiles_match_whole(out, whole[1], q, f"{route} tiles {T} ({first}, {stride}) schedule {team}")
                assert _stats(out[3]) == _stats(tiled[1][3]), (route, T, first, stride, team)
        assert n_tiled > 0
        return st


@pytest.fixture(scope="module")
def rigs(rig, rig16):
    return Rigs(lego=rig, aabb16=rig16)


@pytest.mark.gpu
@pytest.mark.parametrize("route", list(ROUTES))
def test_route(rigs, route):
    st = render_route(rigs, route)
    assert st.n_samples > 10000


@pytest.mark.gpu
def test_affine_with_forced_lane_teams_on_tiles(rigs):
    """the ADVICE r6 bug: AffineDuplication with nrs_ctx_set_lane_teams(2 | 4) on tiles -- packets sized for 8x4 / 4x4 while the one-lane AFFINE
    instantiation ran; now nrs_render_nerf runs it with one lane per ray: bit-equal to the whole image, the sentinel tail intact"""
    with route_on(rigs, "R5_cage_affine") as (rig, _, p):
        rig.ctx.set_lane_teams(1)
        whole = guarded_render(rig, p)
        for team in (2, 4):
            for T, first, stride in TILINGS:
                q = _with(p, tile_size=T, tile_first=first, tile_stride=stride)
                rig.ctx.set_lane_teams(team)
                out = guarded_render(rig, q)
                assert assert_tiles_match_whole(out, whole, q, f"affine, {team} lanes per ray, tiles {T}") > 0


@pytest.mark.gpu
def test_every_reachable_instantiation_is_rendered(tmp_path):
    """the matrix's renders in a child process with the kernel log on (NRS_DEV_KNOBS=1 NRS_KERNEL_LOG=1 in its environment only): the set of
    instantiations launched equals the list above of every instantiation plan_route can reach without development knobs -- a route added
    without a test here fails this"""
    env = dict(os.environ, NRS_DEV_KNOBS="1", NRS_KERNEL_LOG="1")
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "route_worker.py")], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                        text=True, timeout=600)
    assert pr.returncode == 0, (pr.stdout[-2000:], pr.stderr[-4000:])
    assert "routes rendered: %d" % len(ROUTES) in pr.stdout, pr.stdout[-2000:]
    seen = set(re.findall(r"^\[nrs kernel\] (.*)$", pr.stderr, re.M))
    expected = expected_instantiations()
    ran = {}
    for names in expected:
        hit = [n for n in names if n in seen]
        assert hit, f"never launched: {names[0]}"
        ran[names[0]] = hit
    accepted = {n for names in expected for n in names}
    extra = sorted(seen - accepted)
    assert not extra, f"launched but not in the list of reachable instantiations: {extra}"
    for names in expected:
        if len(names) > 1:
            print(f"{names[0]}: ran {' and '.join('the 128-register entry point' if n.startswith('render_kernel_c128') else 'its (512, 4) twin' for n in ran[names[0]])}")
