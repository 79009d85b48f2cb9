"""The cameras of render_to_cpu's loop on the host (nrs_log_space_lerp, nrs_camera_keyframe_*, nrs_camera_path_*, nrs_motion_views) against float64 restatements
written here.  No GPU.  Every bound is a rounding bound derived from the formula, not a measurement:

  log_space_lerp      the library evaluates in double and rounds once: |got - want| <= 2^-23 max(1, max|want|) per entry (one float32 rounding, factor 2);
  camera_path_eval    float arithmetic as the reference's: per component 16 * 2^-24 * sum_i |w_i k_i| (a weight carries <= 6 roundings, one product, three additions);
  keyframe_matrix     entries <= 1 from a short chain: 16 * 2^-24 per entry, and the same for matrix -> keyframe -> matrix;
  motion_views        matrices identical to nrs_log_space_lerp's, focal length / dof / slice within 2 float32 ulp of the float64 values."""
import ctypes as C
import json

import numpy as np
import pytest
from scipy.linalg import expm, logm

from nerfshop_amd import _abi
from nerfshop_amd._abi import CameraKeyframe, SampleView

F12 = C.c_float * 12
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def lib(built):
    return _abi.load()


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def to12(R, T):
    """3x3 and translation -> the 3x4 column-major [12] float32 layout of the header"""
    return np.concatenate([np.asarray(R).T.reshape(-1), np.asarray(T)]).astype(np.float32)


def to44(m12):
    A = np.eye(4)
    A[:3, :] = np.asarray(m12, np.float64).reshape(4, 3).T
    return A


def lerp(lib, a, b, t):
    out = F12()
    st = lib.nrs_log_space_lerp(C.byref(F12(*a)), C.byref(F12(*b)), float(t), C.byref(out))
    assert st == 0, lib.nrs_last_error()
    return np.array(out, np.float32)


def camera_pairs():
    """200 seeded pairs of rigid cameras: relative rotation up to 170 degrees, translations up to 4; twenty with the NeRF-to-ngp scale 0.33 on the rotation block"""
    rng = np.random.default_rng(20260)
    for i in range(200):
        scale = 0.33 if i < 20 else 1.0
        Ra = rotation(rng.normal(size=3), rng.uniform(0, np.pi))
        angle = np.deg2rad(170.0) if i % 25 == 0 else np.deg2rad(rng.uniform(0.0, 170.0))
        Rb = rotation(rng.normal(size=3), angle) @ Ra
        yield to12(scale * Ra, rng.uniform(-4, 4, 3)), to12(scale * Rb, rng.uniform(-4, 4, 3)), float(np.float32(rng.uniform(0, 1)))


def test_log_space_lerp_against_scipy(lib):
    for a, b, t in camera_pairs():
        A, B = to44(a), to44(b)
        L = logm(B @ np.linalg.inv(A))
        assert np.abs(np.imag(L)).max() < 1e-9
        L = np.real(L)
        for tt, exact in ((t, None), (0.0, a), (1.0, b)):
            want = (expm(tt * L) @ A)[:3, :].T.reshape(-1)
            got = lerp(lib, a, b, tt).astype(np.float64)
            bound = 2.0 ** -23 * max(1.0, np.abs(want).max())
            assert np.abs(got - want).max() <= bound, (tt, np.abs(got - want).max(), bound)
            if exact is not None:
                assert np.abs(got - exact.astype(np.float64)).max() <= bound
        assert np.array_equal(lerp(lib, a, a, t).view(np.uint32), a.view(np.uint32)), "begin == end is returned exactly"


def test_log_space_lerp_refusals(lib):
    a = to12(np.eye(3), (0, 0, 0))
    out = F12()
    bad = a.copy(); bad[3] = np.nan
    assert lib.nrs_log_space_lerp(C.byref(F12(*bad)), C.byref(F12(*a)), 0.5, C.byref(out)) == -1
    singular = to12(np.zeros((3, 3)), (0, 0, 0))
    assert lib.nrs_log_space_lerp(C.byref(F12(*singular)), C.byref(F12(*a)), 0.5, C.byref(out)) == -1 and b"singular" in lib.nrs_last_error()
    half_turn = to12(rotation((0, 0, 1), np.pi), (0, 0, 0))
    half_turn[np.abs(half_turn) < 1e-6] = 0.0
    assert lib.nrs_log_space_lerp(C.byref(F12(*a)), C.byref(F12(*half_turn)), 0.5, C.byref(out)) == -2   # NRS_ERR_UNSUPPORTED: no real logarithm
    assert lib.nrs_log_space_lerp(None, C.byref(F12(*a)), 0.5, C.byref(out)) == -1


# ---- keyframes ---------------------------------------------------------------------------------------------------------------------------------------
def key_of(R4, T, slice_, scale, fov, dof):
    k = CameraKeyframe()
    k.R[:] = [float(v) for v in R4]; k.T[:] = [float(v) for v in T]
    k.slice, k.scale, k.fov, k.dof = slice_, scale, fov, dof
    return k


def quat_matrix64(q):
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(np.asarray(q, np.float64))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def test_keyframe_matrix_and_round_trip(lib):
    rng = np.random.default_rng(7)
    quats = [rng.normal(size=4) * rng.uniform(0.2, 3.0) for _ in range(60)]   # (not normalised: m() normalises)
    quats += [(0, 0, 0, 1), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0.5, 0.5, 0.5, -0.5), (0.7, 0.0, 0.7, 1e-4)]   # every branch of the matrix -> quaternion conversion
    for q in quats:
        q32 = np.asarray(q, np.float32)
        T = rng.uniform(-4, 4, 3).astype(np.float32)
        k = key_of(q32, T, 0.1, 1.0, 50.0, 0.0)
        m = F12()
        assert lib.nrs_camera_keyframe_matrix(C.byref(k), C.byref(m)) == 0
        m = np.array(m, np.float32)
        want = quat_matrix64(q32.astype(np.float64))
        assert np.abs(m[:9].astype(np.float64).reshape(3, 3).T - want).max() <= 16 * EPS
        assert np.array_equal(m[9:], T)
        back = CameraKeyframe()
        assert lib.nrs_camera_keyframe_from_matrix(C.byref(F12(*m)), 0.25, 1.5, 40.0, 0.01, C.byref(back)) == 0
        assert (back.slice, back.scale, back.fov, back.dof) == (0.25, 1.5, 40.0, float(np.float32(0.01))) and list(back.T) == list(T)
        assert abs(np.linalg.norm(np.array(back.R, np.float64)) - 1.0) <= 16 * EPS
        m2 = F12()
        assert lib.nrs_camera_keyframe_matrix(C.byref(back), C.byref(m2)) == 0
        assert np.abs(np.array(m2, np.float64) - m.astype(np.float64)).max() <= 16 * EPS


def spline64(keys, t):
    """CameraPath::eval_camera_path + spline (the cubic B-spline) in float64 with operator+'s sign flips -> (value [11], sum_i |w_i k_i| [11], the number of flips)"""
    n = len(keys)
    t = np.float64(np.float32(t) * np.float32(n - 1))   # (the float product is the reference's own argument)
    t1 = int(np.floor(t))
    s = t - np.floor(t)
    w = [(1 - s) ** 3 / 6.0, (3 * s ** 3 - 6 * s ** 2 + 4) / 6.0, (-3 * s ** 3 + 3 * s ** 2 + 3 * s + 1) / 6.0, s ** 3 / 6.0]
    vec = lambda k: np.array(list(k.R) + list(k.T) + [k.slice, k.scale, k.fov, k.dof], np.float64)
    ps = [vec(keys[min(max(t1 + o, 0), n - 1)]) for o in (-1, 0, 1, 2)]
    acc = ps[0] * w[0]
    mag = np.abs(acc)
    n_flips = 0
    for p, wi in zip(ps[1:], w[1:]):
        term = p * wi
        if np.dot(term[:4], acc[:4]) < 0:
            term[:4] = -term[:4]
            n_flips += 1
        acc = acc + term
        mag = mag + np.abs(term)
    return acc, mag, n_flips


@pytest.mark.parametrize("n", [2, 3, 7])
def test_camera_path_eval(lib, n):
    rng = np.random.default_rng(100 + n)
    keys = []
    for i in range(n):
        q = rotation((0.2, 1.0, 0.1), 0.5 * i)
        k = CameraKeyframe()
        m = F12(*to12(q, rng.uniform(-2, 2, 3)))
        assert lib.nrs_camera_keyframe_from_matrix(C.byref(m), float(rng.uniform(-0.5, 0.5)), float(rng.uniform(0.5, 2)), float(rng.uniform(20, 90)), float(rng.uniform(0, 0.1)), C.byref(k)) == 0
        if i % 2:   # the opposite-sign quaternion of the same rotation: operator+ flips it back
            k.R[:] = [-v for v in k.R]
        keys.append(k)
    arr = (CameraKeyframe * n)(*keys)
    knots = [i / (n - 1) for i in range(n)]
    ts = [0.0, 1.0] + knots + [(a + b) / 2 for a, b in zip(knots, knots[1:])] + [float(x) for x in rng.uniform(0, 1, 12)] + [0.999999, 1e-7]
    flips = 0
    for t in ts:
        out = CameraKeyframe()
        assert lib.nrs_camera_path_eval(C.cast(arr, C.c_void_p), n, float(np.float32(t)), C.byref(out)) == 0
        got = np.array(list(out.R) + list(out.T) + [out.slice, out.scale, out.fov, out.dof], np.float64)
        want, mag, n_flips = spline64(keys, np.float32(t))
        assert (np.abs(got - want) <= 16 * EPS * mag + 1e-45).all(), (t, got - want)
        flips += n_flips
    assert flips > 0, "no evaluation met a quaternion of the opposite sign: the sign flip of operator+ went untested"
    # nothing to evaluate: the default keyframe
    out = key_of((1, 1, 1, 1), (1, 1, 1), 1, 1, 1, 1)
    assert lib.nrs_camera_path_eval(None, 0, 0.5, C.byref(out)) == 0 and list(out.R) == [0.0] * 4 and out.fov == 0.0
    assert lib.nrs_camera_path_eval(C.cast(arr, C.c_void_p), n, float("nan"), C.byref(out)) == -1


# ---- the path file -----------------------------------------------------------------------------------------------------------------------------------
def write_path(path, keys, drop=None):
    rows = []
    for k in keys:
        row = {"R": [float(v) for v in k.R], "T": [float(v) for v in k.T], "slice": float(k.slice), "scale": float(k.scale), "fov": float(k.fov), "dof": float(k.dof)}
        if drop:
            del row[drop]
        rows.append(row)
    path.write_text(json.dumps({"time": 0.25, "path": rows}))   # (CameraPath::save's shape; a float32 prints as the double it converts to: it reads back exactly)


def open_path(lib, path):
    h = C.c_void_p()
    st = lib.nrs_camera_path_open(str(path).encode(), C.byref(h))
    return st, h


def test_camera_path_file(lib, tmp_path):
    rng = np.random.default_rng(3)
    keys = [key_of(rng.normal(size=4).astype(np.float32), rng.normal(size=3).astype(np.float32), *[float(np.float32(v)) for v in rng.normal(size=4)]) for _ in range(5)]
    f = tmp_path / "base_cam.json"
    write_path(f, keys)
    st, h = open_path(lib, f)
    assert st == 0, lib.nrs_last_error()
    try:
        assert lib.nrs_camera_path_count(h) == 5
        out = (CameraKeyframe * 5)()
        assert lib.nrs_camera_path_keyframes(h, C.cast(out, C.c_void_p), 4) == -1 and b"capacity" in lib.nrs_last_error()
        assert lib.nrs_camera_path_keyframes(h, C.cast(out, C.c_void_p), 5) == 0
        assert bytes(out) == bytes((CameraKeyframe * 5)(*keys)), "the keyframes read back bit for bit"
    finally:
        lib.nrs_camera_path_close(h)
    for key in ("R", "T", "slice", "scale", "fov", "dof"):
        write_path(f, keys, drop=key)
        st, h = open_path(lib, f)
        assert st == -1 and f'"{key}"'.encode() in lib.nrs_last_error(), (key, lib.nrs_last_error())
    for text in ('{"time": 0.0, "path": []}', '{"time": 0.0, "path": null}', '{"time": 0.0}'):
        f.write_text(text)
        st, h = open_path(lib, f)
        assert st == 0 and lib.nrs_camera_path_count(h) == 0
        assert lib.nrs_camera_path_keyframes(h, None, 0) == 0
        lib.nrs_camera_path_close(h)
    st, h = open_path(lib, tmp_path / "missing.json")
    assert st == -1 and b"missing.json" in lib.nrs_last_error()


# ---- nrs_motion_views ----------------------------------------------------------------------------------------------------------------------------------
def motion_views(lib, start, end, shutter, count, first, total, res, axis, keys, t0, t1, base):
    out = (SampleView * count)()
    arr = (CameraKeyframe * max(len(keys), 1))(*keys)
    st = lib.nrs_motion_views(C.byref(F12(*start)), C.byref(F12(*end)), shutter, count, first, total, C.byref((C.c_int32 * 2)(*res)), axis,
                              C.cast(arr, C.c_void_p) if keys else None, len(keys), t0, t1, C.byref(base), C.cast(out, C.c_void_p))
    assert st == 0, lib.nrs_last_error()
    return out


def ulps(a, b):
    """distance of the float32 `a` from the float64 `b` in float32 ulps of b"""
    return abs(float(a) - b) / np.spacing(np.float32(abs(b)) if b else np.float32(1e-45))


def test_motion_views(lib):
    f32 = np.float32
    a, b, _ = next(iter(camera_pairs()))
    rng = np.random.default_rng(9)
    keys = []
    for i in range(4):
        k = CameraKeyframe()
        m = F12(*to12(rotation((0, 1, 0), 0.3 * i), rng.uniform(-1, 1, 3)))
        assert lib.nrs_camera_keyframe_from_matrix(C.byref(m), 0.1 * i, 1.0 + 0.1 * i, 40.0 + 5.0 * i, 0.01 * i, C.byref(k)) == 0
        keys.append(k)
    base = SampleView()
    base.focal_length[:] = (111.0, 113.0)
    base.dof, base.slice_plane_z = 0.02, 1.3
    res, total, shutter = (173, 131), 7, f32(0.5)
    for use_path, t0, t1 in ((False, -1.0, -1.0), (True, 0.25, 0.3), (False, 0.25, 0.3)):
        ks = keys if (use_path or t0 < 0) else []   # (a path with start_time < 0, and a start_time without a path: both take the base view)
        for first, count in ((0, 7), (2, 3)):
            views = motion_views(lib, a, b, float(shutter), count, first, total, res, 1, ks, t0, t1, base)
            for j in range(count):
                i = first + j
                a0 = f32(i) / f32(total) * shutter
                a1 = (f32(i) + f32(1.0)) / f32(total) * shutter
                assert np.array_equal(np.array(views[j].camera_matrix0, f32).view(np.uint32), lerp(lib, a, b, a0).view(np.uint32))
                assert np.array_equal(np.array(views[j].camera_matrix1, f32).view(np.uint32), lerp(lib, a, b, a1).view(np.uint32))
                if use_path:
                    t = f32(t0) + (f32(t1) - f32(t0)) * (a0 + a1) / f32(2.0)
                    key = CameraKeyframe()
                    assert lib.nrs_camera_path_eval(C.cast((CameraKeyframe * 4)(*keys), C.c_void_p), 4, float(t), C.byref(key)) == 0
                    focal = 0.5 / np.tan(0.5 * np.float64(key.fov) * np.pi / 180.0) * res[1]
                    assert ulps(views[j].focal_length[0], focal) <= 2 and views[j].focal_length[0] == views[j].focal_length[1]
                    assert ulps(views[j].dof, np.float64(key.dof)) <= 2
                    assert ulps(views[j].slice_plane_z, np.float64(key.slice) + np.float64(key.scale)) <= 2
                else:
                    assert tuple(views[j].focal_length) == (111.0, 113.0) and views[j].dof == base.dof and views[j].slice_plane_z == base.slice_plane_z
    still = motion_views(lib, a, b, 0.0, 5, 0, 5, res, 1, [], -1.0, -1.0, base)
    for v in still:
        assert np.array_equal(np.array(v.camera_matrix0, f32).view(np.uint32), a.view(np.uint32)) and np.array_equal(np.array(v.camera_matrix1, f32).view(np.uint32), a.view(np.uint32))
    out = (SampleView * 2)()
    assert lib.nrs_motion_views(C.byref(F12(*a)), C.byref(F12(*b)), 0.5, 2, 4, 5, None, 1, None, 0, -1.0, -1.0, C.byref(base), C.cast(out, C.c_void_p)) == -1
    assert b"spp_total" in lib.nrs_last_error()


def test_sample_view_layout():
    assert C.sizeof(SampleView) == 112 and C.sizeof(CameraKeyframe) == 44
