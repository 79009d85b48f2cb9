"""The C++ face of the camera path (include/nrs_compat.hpp: Testbed::load_camera_path, set_camera_from_time, apply_camera_smoothing; render_to_cpu is compiled with them):
a small host program over the header, built -Wall -Wextra -Werror like examples/, run on the CPU -- the camera functions of libnrs.so need no GPU -- and compared bit for
bit with the same calls made through ctypes.  No GPU."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
TIMES = (0.0, 0.3, 0.55, 1.0)
FPS = 24.0

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include "nrs_compat.hpp"
static void put(const float* v, int n) { for (int i = 0; i < n; ++i) { unsigned u; memcpy(&u, v + i, 4); printf("%08x ", u); } printf("\n"); }
int main(int argc, char** argv) {
	if (argc < 2) return 2;
	auto render_to_cpu = &nrs::compat::Testbed::render_to_cpu; // (instantiates it: the header compiles under -Werror with its GPU path too)
	if (!render_to_cpu) return 3;
	nrs::compat::Testbed tb;
	tb.set_camera_from_time(0.5f); // no keyframes: nothing happens
	put(tb.m_camera, 12);
	tb.load_camera_path(argv[1]);
	printf("%zu\n", tb.m_camera_path.size());
	const float times[4] = {0.0f, 0.3f, 0.55f, 1.0f};
	for (float t : times) {
		tb.set_camera_from_time(t);
		put(tb.m_camera, 12);
		const float rest[4] = {tb.m_slice_plane_z, tb.m_scale, tb.m_fov, tb.m_dof};
		put(rest, 4);
	}
	tb.set_camera_from_time(0.0f);
	tb.apply_camera_smoothing(1000.f / 24.f); // smoothing off: the smoothed camera IS the camera
	put(tb.m_smoothed_camera, 12);
	tb.m_camera_smoothing = true;
	tb.set_camera_from_time(1.0f);
	tb.apply_camera_smoothing(1000.f / 24.f);
	put(tb.m_smoothed_camera, 12);
	float focal[2];
	tb.calc_focal_length(160, 90, focal);
	put(focal, 2);
	try { tb.load_camera_path("/nonexistent/path.json"); return 4; } catch (const std::runtime_error&) {}
	return 0;
}
"""


def words(line):
    return np.array([int(w, 16) for w in line.split()], np.uint32).view(np.float32)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_compat_camera_path_and_smoothing(tmp_path):
    from nerfshop_amd import _abi
    from nerfshop_amd._abi import CameraKeyframe
    lib = _abi.load()
    F12 = C.c_float * 12
    rng = np.random.default_rng(3)
    keys = []
    for i in range(4):
        a = 0.4 * i
        m = F12(np.cos(a), 0.0, -np.sin(a), 0.0, 1.0, 0.0, np.sin(a), 0.0, np.cos(a), *[float(v) for v in rng.uniform(-1, 1, 3)])
        k = CameraKeyframe()
        assert lib.nrs_camera_keyframe_from_matrix(C.byref(m), 0.1 * i, 1.0 + 0.1 * i, 40.0 + 5.0 * i, 0.01 * i, C.byref(k)) == 0
        keys.append(k)
    path = tmp_path / "path.json"
    path.write_text(json.dumps({"time": 0.0, "path": [{"R": [float(v) for v in k.R], "T": [float(v) for v in k.T], "slice": float(k.slice), "scale": float(k.scale),
                                                        "fov": float(k.fov), "dof": float(k.dof)} for k in keys]}))
    src, exe = tmp_path / "host.cpp", tmp_path / "host"
    src.write_text(PROGRAM)
    libdir = os.path.join(ROOT, "nerfshop_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src),
                           "-L", libdir, "-lnrs", "-L", os.path.join(ROCM, "lib"), "-lamdhip64", f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{os.path.join(ROCM, 'lib')}"])
    lines = subprocess.run([str(exe), str(path)], check=True, capture_output=True, text=True, timeout=60).stdout.strip().split("\n")
    assert list(words(lines[0])) == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0] and int(lines[1]) == 4

    arr = (CameraKeyframe * 4)(*keys)

    def camera_at(t):
        k, m = CameraKeyframe(), F12()
        assert lib.nrs_camera_path_eval(C.cast(arr, C.c_void_p), 4, float(np.float32(t)), C.byref(k)) == 0
        assert lib.nrs_camera_keyframe_matrix(C.byref(k), C.byref(m)) == 0
        return np.array(m, np.float32), k

    for i, t in enumerate(TIMES):
        m, k = camera_at(t)
        assert np.array_equal(words(lines[2 + 2 * i]).view(np.uint32), m.view(np.uint32)), t
        assert np.array_equal(words(lines[3 + 2 * i]), np.array([k.slice, k.scale, k.fov, k.dof], np.float32)), t
    first, last = camera_at(0.0)[0], camera_at(1.0)
    assert np.array_equal(words(lines[10]).view(np.uint32), first.view(np.uint32))
    # testbed.cu:2086-2093: decay = pow(0.02f, elapsed_ms / 1000), smoothed = log_space_lerp(smoothed, camera, 1 - decay)
    decay = np.float32(0.02) ** (np.float32(1000.0) / np.float32(FPS) / np.float32(1000.0))
    out = F12()
    assert lib.nrs_log_space_lerp(C.byref(F12(*first)), C.byref(F12(*last[0])), float(np.float32(1.0) - decay), C.byref(out)) == 0
    got = words(lines[11])
    assert not np.array_equal(got, first) and not np.array_equal(got, last[0])
    # (powf of the C library against numpy's: at most one unit in the last place of the lerp's argument, which moves a camera entry of magnitude <= 4 by no more than 2^-21)
    assert np.abs(got.astype(np.float64) - np.array(out, np.float64)).max() <= 2.0 ** -21
    rel = 0.5 / np.tan(0.5 * np.float64(last[1].fov) * np.pi / 180.0)
    assert np.array_equal(words(lines[12]), np.full(2, np.float32(rel * 90.0)))
