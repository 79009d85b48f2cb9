"""The C++ face of the environment map (include/nrs_compat.hpp: nrs::compat::Envmap, NerfNetwork::ray_loss_ex): a small host program over the header, built -Wall
-Wextra -Werror like examples/, run on the CPU.  Its host-only parts -- the default optimiser, the accumulate parameters taken from a ray loss's, the schedule, the
layouts the header promises -- are checked against the ctypes mirror; every member is instantiated so that the header compiles with its GPU path too.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

PROGRAM = r"""
#include <cstddef>
#include <cstdio>
#include <cstring>
#include "nrs_compat.hpp"
int main() {
	using nrs::compat::Envmap;
	using nrs::compat::NerfNetwork;
	auto set_texels = &Envmap::set_texels; void (Envmap::*get)(nrs_envmap_what, void*) = &Envmap::get; auto export_texels = &Envmap::export_texels; auto background = &Envmap::background;
	auto accumulate = &Envmap::accumulate; auto n_floats = &Envmap::n_floats; auto ray_loss_ex = &NerfNetwork::ray_loss_ex;
	void (Envmap::*step)(void*, float, float) = &Envmap::step;   // (instantiates them: the header compiles under -Werror with its GPU path too)
	uint32_t (Envmap::*step_count)() const = &Envmap::step;
	if (!set_texels || !get || !export_texels || !background || !accumulate || !n_floats || !ray_loss_ex || !step || !step_count) return 3;
	const nrs_adam_params p = Envmap::base_params();
	printf("%u %zu %.9g %.9g %.9g %.9g %.9g %.9g\n", p.struct_size, sizeof(nrs_adam_params), p.beta1, p.beta2, p.epsilon, p.l2_reg, p.non_matrix_lr_factor, p.ema_decay);
	nrs_ray_loss_params loss{};
	loss.struct_size = (uint32_t)sizeof(loss); loss.loss_type = NRS_LOSS_HUBER; loss.loss_scale = 64.f; loss.train_in_linear_colors = 1;
	const nrs_envmap_accumulate_params a = Envmap::accumulate_params(loss);
	printf("%u %zu %u %u %.9g %u %u\n", a.struct_size, sizeof(a), a.loss_type, a.envmap_loss_type, a.loss_scale, a.train_in_linear_colors, (unsigned)NRS_RAY_AUX_WORDS);
	printf("%.9g %.9g %.9g %.9g\n", Envmap::envmap_lr(0), Envmap::envmap_lr(9999), Envmap::envmap_lr(10000), Envmap::envmap_lr(15000));
	// refused by name before any device is touched (the handle of zeros is never read)
	unsigned char zeros[1024];
	memset(zeros, 0, sizeof(zeros));
	nrs_envmap* out = nullptr;
	if (nrs_envmap_create((nrs_ctx*)zeros, 0, 4, nullptr, &out) != NRS_ERR_INVALID_ARG || !strstr(nrs_last_error(), "resolution") || out) return 4;
	nrs_envmap_accumulate_params bad = a;
	bad.envmap_loss_type = 99;
	if (nrs_envmap_accumulate((nrs_envmap*)zeros, nullptr, &bad, 0, nullptr, nullptr, nullptr, nullptr, nullptr) != NRS_ERR_INVALID_ARG || !strstr(nrs_last_error(), "loss_type")) return 5;
	if (nrs_envmap_accumulate((nrs_envmap*)zeros, nullptr, &a, 0, nullptr, nullptr, nullptr, nullptr, nullptr) != NRS_OK) return 6;
	if (nrs_envmap_step((nrs_envmap*)zeros, nullptr, 0.f, 1e-2f) != NRS_ERR_INVALID_ARG || !strstr(nrs_last_error(), "loss_scale")) return 7;
	return 0;
}
"""


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_compat_envmap_host_parts(built, tmp_path):
    from nerfshop_amd import _abi
    src, exe = tmp_path / "host.cpp", tmp_path / "host"
    src.write_text(PROGRAM)
    libdir = os.path.join(ROOT, "nerfshop_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src),
                           "-L", libdir, "-lnrs", "-L", os.path.join(ROCM, "lib"), "-lamdhip64", f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{os.path.join(ROCM, 'lib')}"])
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.strip().split("\n")
    f32 = np.float32
    q = _abi.envmap_adam_params()
    want = [C.sizeof(_abi.AdamParams), C.sizeof(_abi.AdamParams), q.beta1, q.beta2, q.epsilon, q.l2_reg, q.non_matrix_lr_factor, q.ema_decay]
    assert [float(f32(float(v))) for v in lines[0].split()] == [float(f32(v)) for v in want]   # (%.9g round-trips a float32)
    assert (q.beta1, q.beta2, q.epsilon, q.ema_decay) == (f32(0.9), f32(0.99), f32(1e-10), f32(0.99)), "base.json's envmap block"
    A = _abi.EnvmapAccumulateParams
    assert [float(v) for v in lines[1].split()] == [C.sizeof(A), C.sizeof(A), _abi.LOSS_HUBER, _abi.LOSS_RELATIVE_L2, 64.0, 1, _abi.RAY_AUX_WORDS]
    lib = _abi.load()
    lr = [float(lib.nrs_exponential_decay_lr(_abi.ENVMAP_LEARNING_RATE, _abi.ENVMAP_DECAY_START, _abi.ENVMAP_DECAY_INTERVAL, _abi.ENVMAP_DECAY_BASE, s)) for s in (0, 9999, 10000, 15000)]
    assert [float(f32(float(v))) for v in lines[2].split()] == lr and lr[0] == lr[1] == float(f32(1e-2)) and lr[2] == float(f32(0.33e-2)) and lr[3] < lr[2]
