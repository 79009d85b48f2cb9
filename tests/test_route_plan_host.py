"""The route planner (nerfshop_amd/csrc/nrs_route.h plan_route) on the CPU: every request is refused for a documented reason or gets a row of the
instantiation table whose traits serve it -- the conditions launch_render's last guard (nrs_render.hip check_route) states, asked of the plan before any launch.

The planner is reached through nrs_route_probe, a symbol libnrs.so exports for this test alone (declared in nrs_render.h, not part of include/nrs.h);
RouteRequest / RouteProbe below mirror the structs of nrs_route.h / nrs_render.h, and the symbol refuses a mirror whose size has drifted."""
import ctypes as C
import itertools
import re

import numpy as np
import pytest

from test_gpu_route_matrix import C128, CFG, R, REACHABLE_C128, REACHABLE_CFG, ROUTES, SCHEDULES, TILINGS

NRS_OK, NRS_ERR_STATE, NRS_ERR_UNSUPPORTED = 0, -5, -2
AO, SHADE, NORMALS, POSITIONS, DEPTH, DISTANCE, STEPSIZE, DISTORTION, COST, SLICE = range(10)
ENCODING_VIS = 11


class RouteKnobs(C.Structure):
    _fields_ = [("team", C.c_int32), ("hybrid_on", C.c_uint32), ("render_cfg", C.c_int32), ("render_cfg_set", C.c_uint32), ("debug", C.c_uint32),
                ("l2_gate", C.c_uint32), ("tail_target", C.c_uint32), ("tail_every", C.c_uint32), ("tail_fill", C.c_uint32), ("alltail_target", C.c_uint32)]


class RouteRequest(C.Structure):
    _fields_ = [("n_extra_dims", C.c_uint32), ("rgb_deep", C.c_uint32), ("numerics", C.c_uint32), ("hashed_pairs", C.c_int32),
                ("any_poisson", C.c_uint32), ("any_affine", C.c_uint32), ("apply_operators", C.c_uint32),
                ("render_mode", C.c_uint32), ("show_accel", C.c_uint32), ("dof_on", C.c_uint32), ("distortion_mode", C.c_uint32), ("distortion_map", C.c_uint32),
                ("envmap", C.c_uint32), ("glow_mode", C.c_uint32), ("cone_angle_constant", C.c_float),
                ("tile_size", C.c_uint32), ("height", C.c_uint32), ("spp_count", C.c_uint32),
                ("lane_teams", C.c_int32), ("n_cus", C.c_int32), ("busy", C.c_uint32), ("pixels_owned", C.c_uint32), ("hit_share", C.c_double),
                ("knobs", RouteKnobs)]


class RouteProbe(C.Structure):
    _fields_ = [("status", C.c_int32), ("row", C.c_int32), ("team", C.c_uint32), ("all_tail", C.c_uint32), ("fill_lanes", C.c_uint32), ("tail_every", C.c_uint32),
                ("tail_target", C.c_uint32), ("hybrid", C.c_uint32), ("row_has_batch", C.c_uint32), ("name", C.c_char * 96), ("message", C.c_char * 256)]


def _dtype(struct):
    """the numpy view of a ctypes struct (char arrays as byte strings)"""
    def fmt(t):
        return f"S{C.sizeof(t)}" if issubclass(t, C.Array) else np.dtype(t)
    return np.dtype(dict(names=[n for n, _ in struct._fields_], formats=[fmt(t) for _, t in struct._fields_],
                         offsets=[getattr(struct, n).offset for n, _ in struct._fields_], itemsize=C.sizeof(struct)))


REQ, PROBE = np.dtype(RouteRequest), _dtype(RouteProbe)
TRIGGERS = ("show_accel", "dof_on", "distortion_mode", "distortion_map", "envmap", "glow_mode")
NAME = re.compile(r"render_kernel(_c128)?<(\d+)(?:, (\d+))?, prof (\d), poisson (\d), affine (\d), team (\d), num (-?\d), extra (\d)(, batch)?>$")


@pytest.fixture(scope="module")
def probe():
    from nerfshop_amd import _abi
    lib = _abi.load()
    fn = lib.nrs_route_probe
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32]

    def run(requests):
        out = np.zeros(len(requests), PROBE)
        assert fn(requests.ctypes.data, REQ.itemsize, len(requests), out.ctypes.data, PROBE.itemsize) == NRS_OK
        return out
    return run


def blank(n):
    """n requests of a production process: a 173 x 131 frame on a 256-CU GPU, no launch finished yet, default knobs"""
    q = np.zeros(n, REQ)
    q["render_mode"] = SHADE
    q["height"], q["spp_count"], q["n_cus"], q["hit_share"] = 131, 1, 256, 0.25
    q["pixels_owned"] = 22 * 17 * 64
    k = q["knobs"]
    k["hybrid_on"], k["l2_gate"], k["tail_target"], k["tail_every"], k["tail_fill"], k["alltail_target"] = 1, 1, 24, 3, 4, 16
    return q


def test_mirror_is_checked(probe):
    from nerfshop_amd import _abi
    lib = _abi.load()
    q, out = blank(1), np.zeros(1, PROBE)
    assert lib.nrs_route_probe(C.c_void_p(q.ctypes.data), C.c_uint32(REQ.itemsize - 4), C.c_uint32(1), C.c_void_p(out.ctypes.data), C.c_uint32(PROBE.itemsize)) != NRS_OK


def traits_of(names):
    """{name: (c128, waves, occ, prof, poisson, affine, team, num, xtra, batch)} parsed from the rows' names as route_name prints them"""
    out = {}
    for n in names:
        m = NAME.match(n)
        assert m, n
        out[n] = (bool(m.group(1)), int(m.group(2)), int(m.group(3) or 3)) + tuple(int(m.group(i)) for i in range(4, 10)) + (bool(m.group(10)),)
    return out


def inner_axes():
    """the cross product of every axis but the model's and the operators': one template the sweep re-uses per model / operator combination"""
    modes = (SHADE, COST, DEPTH, NORMALS, ENCODING_VIS)
    triggers = (None,) + TRIGGERS
    forced = [(0, 0)] + [(f, 0) for f in (1, 2, 4, -1, -2, -3, -4)] + [(0, f) for f in (1, 2, 4, -1, -2, -3, -4)]  # (lane_teams, NRS_TEAM)
    axes = list(itertools.product(modes, triggers, (0, 1), forced, (1, 0), (0, 32), (1, 2), (0, 1), (0, 84, 42, 124)))
    q = blank(len(axes))
    cols = list(zip(*axes))
    q["render_mode"] = cols[0]
    for t in TRIGGERS:
        q[t] = [1 if x == t else 0 for x in cols[1]]
    gate = np.array(cols[2])
    q["cone_angle_constant"] = np.where(gate, 1.0 / 256.0, 0.0)
    q["hashed_pairs"] = np.where(gate, 3, 0)
    q["lane_teams"] = [f[0] for f in cols[3]]
    q["knobs"]["team"] = [f[1] for f in cols[3]]
    q["knobs"]["hybrid_on"] = cols[4]
    q["tile_size"] = cols[5]
    tiled = np.array(cols[5]) != 0
    q["pixels_owned"] = np.where(tiled, 5 * 32 * 32, 22 * 17 * 64)
    q["spp_count"] = cols[6]
    q["pixels_owned"] *= q["spp_count"]
    q["knobs"]["debug"] = np.array(cols[7]) * 4
    q["knobs"]["render_cfg"] = cols[8]
    q["knobs"]["render_cfg_set"] = np.array(cols[8]) != 0
    return q


def test_every_request_is_refused_or_served(probe):
    """the full cross product: model kind x numerics x operators x modes and EXTRA triggers x gate x forced schedules (both ways) x NRS_HYBRID x tiles x batch x
    wave log x NRS_RENDER_CFG"""
    template = inner_axes()
    extra_needed = (~np.isin(template["render_mode"], (SHADE, COST))) | np.any([template[t] != 0 for t in TRIGGERS], axis=0)
    intro = np.isin(template["render_mode"], (NORMALS, ENCODING_VIS))
    gate_ok = template["hashed_pairs"] == 3
    wave_log = template["knobs"]["debug"] != 0
    cfg = template["knobs"]["render_cfg"]
    batch = template["spp_count"] > 1
    n_total, seen_status = 0, set()
    for light, deep, numerics, poisson, affine, apply_ops in itertools.product((0, 1), (0, 1), range(4), (0, 1), (0, 1), (0, 1)):
        q = template.copy()
        q["n_extra_dims"], q["rgb_deep"], q["numerics"], q["any_poisson"], q["any_affine"], q["apply_operators"] = 3 * light, deep, numerics, poisson, affine, apply_ops
        out = probe(q)
        n_total += len(q)
        what = (light, deep, numerics, poisson, affine, apply_ops)
        # refusals: the documented ones, and each of them always
        unsupported = np.full(len(q), bool(light)) & (bool(poisson and apply_ops) | wave_log | (cfg != 0))
        state = ~unsupported & batch & (wave_log | (cfg != 0))
        assert np.array_equal(out["status"] == NRS_ERR_UNSUPPORTED, unsupported), what
        assert np.array_equal(out["status"] == NRS_ERR_STATE, state), what
        ok = out["status"] == NRS_OK
        assert np.array_equal(ok, ~(unsupported | state)), what
        refused = out[~ok]
        assert (refused["row"] == -1).all() and (refused["message"] != b"").all(), what
        seen_status |= set(np.unique(out["status"]).tolist())
        # the rows: traits per row from its name, then check_route's conditions as vectors
        if not ok.any():
            continue
        o, t = out[ok], {k: v[ok] for k, v in dict(extra=extra_needed, intro=intro, gate=gate_ok, log=wave_log, batch=batch).items()}
        _, first, inverse = np.unique(o["row"] * 2 + t["batch"], return_index=True, return_inverse=True)
        names = o["name"][first]
        assert (o["name"] == names[inverse]).all(), what  # (one name per row and twin)
        parsed = traits_of([n.decode() for n in names])
        # (conditions between a row and the model / operators: once per row that occurs; between a row and the request: per request, through `inverse`)
        c128, waves, occ, prof, r_poisson, r_affine, team, num, xtra, r_batch = np.array([parsed[n.decode()] for n in names], np.int64).T
        x_extra, x_intro, x_deep, x_light = np.isin(xtra, (1, 2, 3, 4, 8)), np.isin(xtra, (2, 4, 8)), np.isin(xtra, (3, 4, 5)), np.isin(xtra, (7, 8))
        assert np.isin(team, (0, 1, 2, 4)).all(), what
        assert (r_affine == 1).all() or not affine, what                             # AFFINE covers an AffineDuplication operator
        assert (r_poisson == 1).all() or not (poisson and not light), what            # POISSON covers the membrane correction (a light network's launch drops it: operators off)
        assert ((num == R) | (num == numerics)).all(), what                           # NUM against numerics
        assert (x_light == bool(light)).all(), what                                   # light directions: EXTRA 7 or 8 and only they
        assert ((xtra == 8) | (x_deep == bool(deep))).all(), what                     # a third rgb hidden layer: EXTRA 3..5 and only they
        assert (~x_extra | (team == 1)).all(), what                                   # the EXTRA instantiations are built for one lane per ray
        team, x_extra = team[inverse], x_extra[inverse]
        assert np.array_equal(o["team"], team), what                                  # the packets are sized for the row's TEAM
        assert (x_extra | ~t["extra"]).all(), what                                    # what the request needs of EXTRA, the row has
        assert (~x_extra | t["extra"] | bool(deep) | bool(light)).all(), what        # ... and only a network with its own catch-all gets it unasked
        assert ((xtra != 6)[inverse] | t["gate"]).all(), what                         # GATE only where the request is gate-eligible
        assert (x_intro[inverse] | ~t["intro"]).all(), what                           # Normals / EncodingVis: INTRO
        assert ((prof == 0)[inverse] | t["log"]).all(), what                          # PROF only with the wave log
        assert np.array_equal((r_batch != 0)[inverse], t["batch"]) and (o["row_has_batch"][t["batch"]] == 1).all(), what  # a batch only on a row that has a batch twin
        # the schedule fields agree with the row
        assert ((o["all_tail"] == 0) | (team == 0)).all() and ((o["hybrid"] == 0) | ((team == 0) & (q["tile_size"][ok] == 0))).all(), what
        assert ((team != 0) | ((o["all_tail"] == 1) ^ (o["hybrid"] == 1))).all(), what
        assert ((o["fill_lanes"] == 1) | (o["fill_lanes"] == 2) | (o["fill_lanes"] == 4)).all(), what
    assert n_total == 128 * len(template) and n_total > 300000
    assert seen_status == {NRS_OK, NRS_ERR_STATE, NRS_ERR_UNSUPPORTED}


# ---- the named routes of tests/test_gpu_route_matrix.py ----------------------------------------------------------------------------------------------
def c128(q, a, t, n, x):
    assert (q, a, t, n, x) in REACHABLE_C128
    return C128.format(p=0, q=q, a=a, t=t, n=n, x=x)


def cfg(w, o, q, a, t, n, x):
    assert (w, o, q, a, t, n, x) in REACHABLE_CFG
    return CFG.format(w=w, o=o, p=0, q=q, a=a, t=t, n=n, x=x)


def lanes(schedule, tiled):
    """TEAM of the default kernel's family under a schedule: 0 for the automatic schedules (0, -2, -3, -4) and the hybrid one (-1) on whole images"""
    return schedule if schedule in (1, 2, 4) else (1 if schedule == -1 and tiled else 0)


def catch_all(num, x):
    return lambda s, tiled: cfg(12, 3, 1, 1, 1, num, x)


# route -> (schedule, tiled) -> the row, written out from the comments of the instantiation table (nrs_route.h kRoutes) and the planner's rules
EXPECTED = {
    "R1_noedit": lambda s, tiled: c128(0, 0, lanes(s, tiled), 0, 0),
    "R2_cage": lambda s, tiled: c128(0, 0, lanes(s, tiled), 0, 0),
    # the membrane correction of cage edits alone runs the automatic schedule; forced lanes per ray and the hybrid schedule leave it on the Shade catch-all
    "R3_membrane_t0": lambda s, tiled: cfg(8, 4, 1, 0, 0, 0, 0) if s in (0, -2, -3, -4) else cfg(12, 3, 1, 1, 1, 0, 0),
    "R3_membrane_t1": lambda s, tiled: cfg(8, 4, 1, 0, 0, 0, 0) if s in (0, -2, -3, -4) else cfg(12, 3, 1, 1, 1, 0, 0),
    # AffineDuplication: the automatic schedule, or one lane per ray
    "R4_affine": lambda s, tiled: c128(0, 1, 0, 0, 0) if s in (0, -2, -3, -4) else cfg(8, 4, 0, 1, 1, 0, 0),
    "R5_cage_affine": lambda s, tiled: c128(0, 1, 0, 0, 0) if s in (0, -2, -3, -4) else cfg(8, 4, 0, 1, 1, 0, 0),
    "R6_membrane_affine": lambda s, tiled: cfg(12, 3, 1, 1, 1, 0, 0),
    # numerics: compile-time instantiations where the wave decides, the run-time twin for fixed lanes per ray
    "R7_num11_cage": lambda s, tiled: c128(0, 0, 0, 3, 0) if lanes(s, tiled) == 0 else cfg(8, 3, 0, 0, lanes(s, tiled), R, 0),
    "R8_num10": lambda s, tiled: c128(0, 0, 0, 1, 0) if lanes(s, tiled) == 0 else cfg(8, 3, 0, 0, lanes(s, tiled), R, 0),
    "R8_num01": lambda s, tiled: c128(0, 0, 0, 2, 0) if lanes(s, tiled) == 0 else cfg(8, 3, 0, 0, lanes(s, tiled), R, 0),
    "R9_num11_cage_affine": lambda s, tiled: cfg(8, 3, 0, 1, 1, R, 0),
    # DEEP: its own instantiation on the unforced automatic schedule, the DEEP catch-all under any forced one
    "R10_deep_cage": lambda s, tiled: cfg(8, 4, 0, 0, 0, 0, 5) if s == 0 else cfg(12, 3, 1, 1, 1, 0, 3),
    "R11_gate_cage": lambda s, tiled: c128(0, 0, 0, 0, 6) if lanes(s, tiled) == 0 else c128(0, 0, lanes(s, tiled), 0, 0),
    "R12_depth_cage": lambda s, tiled: c128(0, 0, 1, 0, 1),
    "R13_normals_cage": catch_all(0, 2),
    "R14_depth_membrane_affine": catch_all(0, 1),
    "R15_num11_membrane": lambda s, tiled: cfg(12, 3, 1, 1, 1, R, 0),
    "R16_num11_depth_cage": catch_all(R, 1),
    "R17_num11_normals_cage": catch_all(R, 2),
    "R18_deep_normals_cage": catch_all(0, 4),
    "R19_deep_num11_cage": catch_all(R, 3),
    "R20_deep_num11_normals": catch_all(R, 4),
}
LIGHT_AUTO = C128.format(p=0, q=0, a=0, t=0, n=0, x=7)
LIGHT_ALL = CFG.format(w=12, o=3, p=0, q=0, a=1, t=1, n=R, x=8)


def request_of(spec, schedule, tile_size, light=False):
    q = blank(1)
    kinds = spec.get("edits", ())
    q["any_poisson"] = "membrane" in kinds
    q["any_affine"] = any(k.startswith("affine") for k in kinds)
    q["apply_operators"] = bool(kinds)
    g, m = spec.get("numerics", (0, 0))
    q["numerics"] = g | (m << 1)
    q["rgb_deep"] = spec.get("rig") == "rgb3"
    q["n_extra_dims"] = 3 if light else 0
    if spec.get("rig") == "aabb16":
        q["cone_angle_constant"], q["hashed_pairs"] = 1.0 / 256.0, 3
    q["render_mode"] = spec.get("fields", {}).get("render_mode", SHADE)
    q["lane_teams"] = schedule
    q["tile_size"] = tile_size
    if tile_size:
        q["pixels_owned"] = 3 * tile_size * tile_size
    return q


def test_named_routes_plan_their_rows(probe):
    assert set(EXPECTED) == set(ROUTES)
    planned = set()
    for route, spec in ROUTES.items():
        for schedule in SCHEDULES:
            for tile_size in (0,) + tuple(sorted({t[0] for t in TILINGS})):
                out = probe(request_of(spec, schedule, tile_size))[0]
                assert out["status"] == NRS_OK, (route, schedule, tile_size, out["message"])
                want = EXPECTED[route](schedule, tile_size != 0)
                assert out["name"].decode() == want, (route, schedule, tile_size)
                planned.add(want)
    # a network with light directions: the LIGHT twin for the plain case on the unforced automatic schedule, its catch-all for everything else
    for schedule in SCHEDULES:
        for tile_size in (0, 32):
            for route, plain in (("R1_noedit", True), ("R2_cage", True), ("R4_affine", False), ("R8_num10", False), ("R12_depth_cage", False), ("R13_normals_cage", False)):
                out = probe(request_of(ROUTES[route], schedule, tile_size, light=True))[0]
                want = LIGHT_AUTO if plain and schedule == 0 else LIGHT_ALL
                assert out["status"] == NRS_OK and out["name"].decode() == want, (route, schedule, tile_size, out["name"])
                planned.add(want)
    reachable = {C128.format(p=0, q=q, a=a, t=t, n=n, x=x) for (q, a, t, n, x) in REACHABLE_C128} | \
                {CFG.format(w=w, o=o, p=0, q=q, a=a, t=t, n=n, x=x) for (w, o, q, a, t, n, x) in REACHABLE_CFG}
    assert planned == reachable | {LIGHT_AUTO, LIGHT_ALL}, (sorted(planned - reachable), sorted(reachable - planned))
