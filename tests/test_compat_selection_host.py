"""The C++ face of the selection tool (include/nrs_compat.hpp: GrowingSelection): a small host program over the header, built -Wall -Wextra -Werror like examples/, run on
the CPU -- growing needs no GPU; dilate, erode and extract_fine_mesh are compiled with it and refuse a NULL context -- and compared with the same calls through ctypes."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import selection_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

PROGRAM = r"""
#include <cstdio>
#include "nrs_compat.hpp"
int main() {
	const uint32_t vol = 128u * 128u * 128u;
	std::vector<float> grid((size_t)5 * vol, 0.f);
	// a 5 x 5 x 5 block of dense cells at level 0, Morton indices computed by the library's own lift of level-0 cells
	auto cell = [](uint32_t x, uint32_t y, uint32_t z) {
		uint32_t m = 0;
		for (uint32_t b = 0; b < 7; ++b) m |= ((x >> b) & 1u) << (3 * b) | ((y >> b) & 1u) << (3 * b + 1) | ((z >> b) & 1u) << (3 * b + 2);
		return m;
	};
	for (uint32_t x = 60; x < 65; ++x)
		for (uint32_t y = 30; y < 35; ++y)
			for (uint32_t z = 90; z < 95; ++z) grid[cell(x, y, z)] = 2.f;
	nrs::compat::GrowingSelection sel(nullptr, grid, 1);
	sel.reset_growing({cell(62, 32, 92), vol + 5u, 2u * vol + 7u}, 0); // the seeds above level 0 are dropped
	printf("%u\n", sel.grow_region(sel.m_density_threshold, 0, sel.m_growing_steps));
	printf("%d\n", sel.growing_level());
	for (uint32_t c : sel.selection_cell_idx()) printf("%u ", c);
	printf("\n");
	for (float p : sel.selection_points()) printf("%.9g ", p);
	printf("\n");
	unsigned long set = 0;
	for (uint8_t b : sel.selection_grid_bitfield()) set += (unsigned long)__builtin_popcount(b);
	printf("%lu\n", set);
	sel.upscale_growing();
	printf("%d %zu\n", sel.growing_level(), sel.selection_cell_idx().size());
	int refused = 0;
	try { sel.dilate(); } catch (const std::runtime_error&) { ++refused; }
	try { sel.erode(); } catch (const std::runtime_error&) { ++refused; }
	try { sel.extract_fine_mesh(); } catch (const std::runtime_error&) { ++refused; }
	printf("%d\n", refused);
	return sel.m_selection_mesh == nullptr && sel.m_use_morphological ? 0 : 5;
}
"""


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_compat_growing_selection(built, tmp_path):
    from nerfshop_amd import runtime as rt
    src, exe = tmp_path / "host.cpp", tmp_path / "host"
    src.write_text(PROGRAM)
    libdir = os.path.join(ROOT, "nerfshop_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src),
                           "-L", libdir, "-lnrs", "-L", os.path.join(ROCM, "lib"), "-lamdhip64", f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{os.path.join(ROCM, 'lib')}"])
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.strip().split("\n")

    grid = np.zeros(ref.CASCADES * ref.VOL, np.float32)
    a = np.arange(ref.G)
    block = ((a >= 60) & (a < 65))[:, None, None] & ((a >= 30) & (a < 35))[None, :, None] & ((a >= 90) & (a < 95))[None, None, :]
    grid[ref.morton_of_grid()[block]] = 2.0
    sel = rt.GrowingSelection(None, grid, 1)
    seed = int(ref.morton(62, 32, 92))
    sel.reset_growing([seed, ref.VOL + 5, 2 * ref.VOL + 7], 0)
    assert int(lines[0]) == sel.grow_region(0.01, 0, 10000) and int(lines[1]) == 0
    cells = np.array(lines[2].split(), np.uint32)
    assert np.array_equal(cells, sel.selection_cell_idx) and len(cells) == 1 + 125
    assert np.array_equal(np.array(lines[3].split(), np.float32).reshape(-1, 3), sel.selection_points)
    assert int(lines[4]) == 125
    assert lines[5].split() == ["1", "126"] and int(lines[6]) == 3
