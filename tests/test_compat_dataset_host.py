"""The C++ face of the dataset (include/nrs_compat.hpp: nrs::compat::Dataset): a small host program over the header, built -Wall -Wextra -Werror like examples/, run on
the CPU.  Its host-only parts -- the camera record Dataset::camera() starts from, the layouts the header promises -- are checked against the ctypes mirror; every
member is instantiated so that the header compiles with its GPU path too.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

PROGRAM = r"""
#include <cstddef>
#include <cstdio>
#include <cstring>
#include "nrs_compat.hpp"
int main() {
	using nrs::compat::Dataset;
	auto set_image = &Dataset::set_image; auto get_image = &Dataset::get_image; auto set_camera = &Dataset::set_camera; auto rays = &Dataset::rays;
	auto mark_untrained = &Dataset::mark_untrained;   // (instantiates them: the header compiles under -Werror with its GPU path too)
	if (!set_image || !get_image || !set_camera || !rays || !mark_untrained) return 3;
	const nrs_training_camera c = Dataset::camera();
	printf("%u %zu %zu %zu %zu\n", c.struct_size, sizeof(nrs_training_camera), offsetof(nrs_training_camera, focal_length), offsetof(nrs_training_camera, distortion_mode),
	       sizeof(nrs_dataset_rays_params));
	for (int i = 0; i < 12; ++i) printf("%g %g ", c.xform_start[i], c.xform_end[i]);
	printf("\n%g %g %g %g %u %llu\n", c.principal_point[0], c.principal_point[1], c.focal_length[0], c.rolling_shutter[3], c.distortion_mode, (unsigned long long)NRS_RNG_STEP_DELTA);
	// the identity camera has no focal length yet: refused by name, before any device is touched (the handle of zeros has no image to index)
	unsigned char zeros[512];
	memset(zeros, 0, sizeof(zeros));
	if (nrs_dataset_set_camera((nrs_dataset*)zeros, 0, &c) != NRS_ERR_INVALID_ARG || !strstr(nrs_last_error(), "focal_length")) return 4;
	nrs_training_camera good = c;
	good.focal_length[0] = good.focal_length[1] = 50.f;
	if (nrs_dataset_set_camera((nrs_dataset*)zeros, 0, &good) != NRS_ERR_INVALID_ARG || !strstr(nrs_last_error(), "index")) return 5;
	uint64_t state = 0, inc = 0, again = 0;
	nrs_rng_seed(1337, &state, &inc);
	again = state;
	nrs_rng_advance(&again, inc, 0);
	if (again != state) return 6;
	nrs_rng_advance(&again, inc, NRS_RNG_STEP_DELTA);
	if (again == state) return 7;
	return 0;
}
"""


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_compat_dataset_host_parts(built, tmp_path):
    from nerfshop_amd import _abi
    src, exe = tmp_path / "host.cpp", tmp_path / "host"
    src.write_text(PROGRAM)
    libdir = os.path.join(ROOT, "nerfshop_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src),
                           "-L", libdir, "-lnrs", "-L", os.path.join(ROCM, "lib"), "-lamdhip64", f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{os.path.join(ROCM, 'lib')}"])
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.strip().split("\n")
    T = _abi.TrainingCamera
    assert [int(v) for v in lines[0].split()] == [C.sizeof(T), C.sizeof(T), T.focal_length.offset, T.distortion_mode.offset, C.sizeof(_abi.DatasetRaysParams)]
    identity = [1.0 if i in (0, 4, 8) else 0.0 for i in range(12)]
    assert [float(v) for v in lines[1].split()] == [v for pair in zip(identity, identity) for v in pair]
    assert lines[2].split() == ["0.5", "0.5", "0", "0", "0", str(_abi.RNG_STEP_DELTA)]
