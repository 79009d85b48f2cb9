"""The route planner with a view per sample (nrs_render_nerf_spp_views).  Every BATCH twin carries the view table, so the flag changes no plan -- except on the lean EXTRA
row, whose still batch keeps its twin (4 waves per SIMD) and whose views batch has a row of its own (EXTRA 9).  Over the request sweep of tests/test_route_plan_host.py:
every request that plans a still batch plans a views batch with the same schedule, on the same row unless that row is the lean EXTRA one; every request refused for a
still batch stays refused for the same reason; a single frame's plan does not depend on the flag; and RoutePlan::views is set for a views batch and for nothing else.
No GPU."""
import ctypes as C
import itertools

import numpy as np

from test_route_plan_host import NRS_OK, PROBE, REQ, RouteKnobs, blank, inner_axes, probe  # noqa: F401  (probe: the fixture)

LEAN = b"render_kernel_c128<8, prof 0, poisson 0, affine 0, team 1, num 0, extra 1, batch>"
LEAN_VIEWS = b"render_kernel_c128<8, prof 0, poisson 0, affine 0, team 1, num 0, extra 9, batch>"


class RouteRequestViews(C.Structure):
    """RouteRequest with its 32-bit sample count read as the two halves nrs_route.h declares: spp_count and the views flag"""
    _fields_ = [("n_extra_dims", C.c_uint32), ("rgb_deep", C.c_uint32), ("numerics", C.c_uint32), ("hashed_pairs", C.c_int32),
                ("any_poisson", C.c_uint32), ("any_affine", C.c_uint32), ("apply_operators", C.c_uint32),
                ("render_mode", C.c_uint32), ("show_accel", C.c_uint32), ("dof_on", C.c_uint32), ("distortion_mode", C.c_uint32), ("distortion_map", C.c_uint32),
                ("envmap", C.c_uint32), ("glow_mode", C.c_uint32), ("cone_angle_constant", C.c_float),
                ("tile_size", C.c_uint32), ("height", C.c_uint32), ("spp_count", C.c_uint16), ("views", C.c_uint16),
                ("lane_teams", C.c_int32), ("n_cus", C.c_int32), ("busy", C.c_uint32), ("pixels_owned", C.c_uint32), ("hit_share", C.c_double),
                ("knobs", RouteKnobs)]


REQV = np.dtype(RouteRequestViews)


def views_of(requests):
    from nerfshop_amd import _abi
    lib = _abi.load()
    out = np.zeros(len(requests), np.uint32)
    assert lib.nrs_route_probe_views(C.c_void_p(requests.ctypes.data), C.c_uint32(REQ.itemsize), C.c_uint32(len(requests)), C.c_void_p(out.ctypes.data)) == NRS_OK
    return out


def test_the_mirrors_agree():
    assert REQV.itemsize == REQ.itemsize
    for name in REQ.names:
        assert REQV.fields[name][1] == REQ.fields[name][1], name
    assert REQV.fields["views"][1] == REQ.fields["spp_count"][1] + 2


def test_views_flag_moves_only_the_lean_extra_row(probe):
    template = inner_axes()
    n_batches = n_refused = n_single = n_lean = 0
    for light, deep, numerics, poisson, affine, apply_ops in itertools.product((0, 1), (0, 1), (0, 3), (0, 1), (0, 1), (0, 1)):
        what = (light, deep, numerics, poisson, affine, apply_ops)
        q = template.copy()
        q["n_extra_dims"], q["rgb_deep"], q["numerics"], q["any_poisson"], q["any_affine"], q["apply_operators"] = 3 * light, deep, numerics, poisson, affine, apply_ops
        still = probe(q)
        v = q.view(REQV).copy()
        assert (v["views"] == 0).all() and np.array_equal(v["spp_count"], q["spp_count"])
        v["views"] = 1
        views = probe(v.view(REQ))
        batch = q["spp_count"] > 1
        ok = still["status"] == NRS_OK
        lean = ok & batch & (still["name"] == LEAN)
        # the lean EXTRA row's views batch: its own row, the same schedule
        assert (views["name"][lean] == LEAN_VIEWS).all() and (views["row"][lean] != still["row"][lean]).all(), what
        assert not (views["name"][~lean] == LEAN_VIEWS).any() and not (still["name"] == LEAN_VIEWS).any(), what
        for field in PROBE.names:
            if field not in ("row", "name"):
                assert np.array_equal(still[field], views[field]), (what, field)
        # everything else: every field of the answer -- status, row, name, message, schedule
        assert np.array_equal(still[~lean].view(np.uint8), views[~lean].view(np.uint8)), what
        assert (views["row_has_batch"][batch & ok] == 1).all()
        # RoutePlan::views: a views batch that is served, and nothing else
        assert not views_of(q).any(), what
        assert np.array_equal(views_of(v.view(REQ)) != 0, batch & ok), what
        n_batches += int((batch & ok).sum()); n_refused += int((batch & ~ok).sum()); n_single += int((~batch).sum()); n_lean += int(lean.sum())
    assert n_batches > 10000 and n_refused > 1000 and n_single > 10000 and n_lean > 100
