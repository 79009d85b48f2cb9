"""The C++ face of per-image exposure (include/nrs_compat.hpp: nrs::compat::Exposure): a small host program over the header, built -Wall -Wextra -Werror like
examples/, run on the CPU.  Its host-only parts -- the default parameters, the accumulate parameters taken from a ray loss's, a step of nrs_exposure_step_host -- are
checked against the ctypes mirror and the twin; every member is instantiated so that the header compiles with its GPU path too.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import exposure_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

PROGRAM = r"""
#include <cstddef>
#include <cstdio>
#include <cstring>
#include "nrs_compat.hpp"
int main() {
	using nrs::compat::Exposure;
	auto set = &Exposure::set; void (Exposure::*get)(nrs_exposure_what, void*) = &Exposure::get; auto export_values = &Exposure::export_values; auto targets = &Exposure::targets;
	auto accumulate = &Exposure::accumulate; auto n_images = &Exposure::n_images;
	void (Exposure::*step)(void*, float, float) = &Exposure::step;   // (instantiates them: the header compiles under -Werror with its GPU path too)
	uint32_t (Exposure::*step_count)() const = &Exposure::step;
	if (!set || !get || !export_values || !targets || !accumulate || !n_images || !step || !step_count) return 3;
	const nrs_exposure_params p = Exposure::default_params();
	printf("%u %zu %.9g %.9g %.9g %.9g %u\n", p.struct_size, sizeof(nrs_exposure_params), p.beta1, p.beta2, p.epsilon, p.l2_reg, p.steps_between_updates);
	nrs_ray_loss_params loss{};
	loss.struct_size = (uint32_t)sizeof(loss); loss.loss_type = NRS_LOSS_HUBER; loss.loss_scale = 64.f; loss.train_in_linear_colors = 1;
	const nrs_exposure_accumulate_params a = Exposure::accumulate_params(loss);
	printf("%u %zu %.9g %u\n", a.struct_size, sizeof(a), a.loss_scale, a.train_in_linear_colors);
	// one step of the host twin: two images, the second without rays
	int64_t cells[6] = {3ll << 32, -(1ll << 31), 7, 0, 0, 0};
	float values[6] = {0.25f, -0.5f, 0.125f, 1.f, 0.f, -1.f}, m[6] = {0.01f, -0.02f, 0.f, 0.03f, 0.f, 0.01f}, v[6] = {1e-4f, 4e-4f, 0.f, 9e-4f, 0.f, 1e-4f};
	uint32_t t = 4;
	if (nrs_exposure_step_host(2, &p, 128.f, 1e-2f, cells, values, m, v, &t) != NRS_OK || t != 5) return 8;
	for (int i = 0; i < 6; ++i) printf("%lld %.9g %.9g %.9g\n", (long long)cells[i], values[i], m[i], v[i]);
	// refused by name before any device is touched (the handle of zeros is never used for a HIP call)
	unsigned char zeros[1024];
	memset(zeros, 0, sizeof(zeros));
	nrs_exposure* out = nullptr;
	if (nrs_exposure_create((nrs_ctx*)zeros, 0, nullptr, &out) != NRS_ERR_INVALID_ARG || !strstr(nrs_last_error(), "n_images") || out) return 4;
	nrs_exposure_accumulate_params bad = a;
	bad.loss_scale = 0.f;
	if (nrs_exposure_accumulate((nrs_exposure*)zeros, nullptr, &bad, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != NRS_ERR_INVALID_ARG || !strstr(nrs_last_error(), "loss_scale")) return 5;
	if (nrs_exposure_accumulate((nrs_exposure*)zeros, nullptr, &a, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != NRS_OK) return 6;
	if (nrs_exposure_step((nrs_exposure*)zeros, nullptr, 0.f, 1e-2f) != NRS_ERR_INVALID_ARG || !strstr(nrs_last_error(), "loss_scale")) return 7;
	return 0;
}
"""


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_compat_exposure_host_parts(built, tmp_path):
    from nerfshop_amd import _abi
    src, exe = tmp_path / "host.cpp", tmp_path / "host"
    src.write_text(PROGRAM)
    libdir = os.path.join(ROOT, "nerfshop_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src),
                           "-L", libdir, "-lnrs", "-L", os.path.join(ROCM, "lib"), "-lamdhip64", f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{os.path.join(ROCM, 'lib')}"])
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.strip().split("\n")
    f32 = np.float32
    q = _abi.ExposureParams()
    want = [C.sizeof(_abi.ExposureParams), C.sizeof(_abi.ExposureParams), q.beta1, q.beta2, q.epsilon, q.l2_reg, q.steps_between_updates]
    assert [float(f32(float(x))) for x in lines[0].split()] == [float(f32(x)) for x in want]   # (%.9g round-trips a float32)
    A = _abi.ExposureAccumulateParams
    assert [float(x) for x in lines[1].split()] == [C.sizeof(A), C.sizeof(A), 64.0, 1]
    cells = np.array([3 << 32, -(1 << 31), 7, 0, 0, 0], np.int64)
    values = np.array([0.25, -0.5, 0.125, 1.0, 0.0, -1.0], f32)
    m = np.array([0.01, -0.02, 0.0, 0.03, 0.0, 0.01], f32)
    v = np.array([1e-4, 4e-4, 0.0, 9e-4, 0.0, 1e-4], f32)
    twin = ref.step(cells, values, m, v, 4, 128.0, 1e-2)
    got = np.array([[float(x) for x in line.split()] for line in lines[2:8]])
    assert not got[:, 0].any(), "the cells are zero afterwards"
    for k in (1, 2, 3):
        assert got[:, k].astype(f32).tobytes() == twin[k].reshape(-1).tobytes(), k
