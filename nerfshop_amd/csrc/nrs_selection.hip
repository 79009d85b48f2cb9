// nrs_selection.hip -- the selection tool's device side (gfx950): dilation and erosion of one level of a bitfield, and the 0 / 1 lattice the fine mesh is cut from.
//
//   morph_pack_kernel      one level from Morton order to x-major rows: 128 bits = 4 words per (y, z) row, bit x % 32 of word x / 32.
//   morph_rows_kernel      CorrectMMOperations::dilate / erode (correct_mm_operations.cu:117-187) on rows: one thread per row, 128 cells per operation.
//   morph_unpack_kernel    rows back to Morton order.
//   selection_lattice_kernel  extract_fine_mesh's float lattice (growing_selection.cu:2113-2140) from rows: 1.0 where the bit is set and the cell is not on the grid's shell.
//
// The element is a list of (dy, dz) rows with an x half-width h each (cube: h = r everywhere; sphere: the largest h with h^2 <= r^2 - dy^2 - dz^2).  Dilation by h along
// x distributes over OR and is h steps of dilation by 1 (shift left, shift right, carry across the four words, 0 shifted in at x = 0 and x = 127), so the rows are taken
// in descending order of h: acc = rows of this h | dilate1(acc of the larger h).  Rows outside the grid are skipped: the reference ignores taps outside the grid.
// Erosion is the same walk on the complement -- a cell survives iff no in-grid tap is clear iff the complement's dilation misses it -- which also shifts 1 in at the ends.
// A level is 256 KiB and stays in L2 between the launches; every launch covers it exactly (no tail, no bounds test needed: the grid sizes are static_asserted).
#include <hip/hip_runtime.h>
#include "../../include/nrs.h"
#include "nrs_internal.h"
#include "nrs_launch.h"
#include "nrs_selection.h"
#include "nrs_grid_math.cuh"

namespace nrs {

static_assert(kGrid == 128 && kMorphLevelWords == 65536, "the kernels below index a level as 128 x 128 rows of four words");

// positions of x % 4 = 0..3 inside a Morton word are base + {0, 1, 8, 9}, base = y0 << 1 | z0 << 2 | y1 << 4 (the low five Morton bits are x0 y0 z0 x1 y1)
__device__ __forceinline__ uint32_t morton_word_base(uint32_t y, uint32_t z) { return ((y & 1u) << 1) | ((z & 1u) << 2) | ((y & 2u) << 3); }

__global__ __launch_bounds__(256) void morph_pack_kernel(const uint32_t* __restrict__ morton, uint32_t* __restrict__ rows) {
	const uint32_t t = blockIdx.x * 256u + threadIdx.x; // word t of the rows: (z, y, w)
	const uint32_t w = t & 3u, y = (t >> 2) & 127u, z = t >> 9;
	const uint32_t base = morton_word_base(y, z);
	uint32_t out = 0;
#pragma unroll
	for (uint32_t q = 0; q < 8; ++q) {
		const uint32_t s = morton[morton3D(32u * w + 4u * q, y, z) >> 5] >> base;
		out |= ((s & 3u) | ((s >> 6) & 0xCu)) << (4u * q);
	}
	rows[t] = out;
}

__global__ __launch_bounds__(256) void morph_unpack_kernel(const uint32_t* __restrict__ rows, uint32_t* __restrict__ morton) {
	const uint32_t t = blockIdx.x * 256u + threadIdx.x; // Morton word t: cells 32 t .. 32 t + 31 = 4 x values, 4 y values, 2 z values
	const uint32_t x0 = morton3D_invert(32u * t), y0 = morton3D_invert((32u * t) >> 1), z0 = morton3D_invert((32u * t) >> 2);
	uint32_t out = 0;
#pragma unroll
	for (uint32_t zz = 0; zz < 2; ++zz)
#pragma unroll
		for (uint32_t yy = 0; yy < 4; ++yy) {
			const uint32_t four = (rows[((z0 + zz) * kGrid + y0 + yy) * 4u + (x0 >> 5)] >> (x0 & 31u)) & 0xFu;
			out |= ((four & 3u) | ((four & 0xCu) << 6)) << morton_word_base(yy, zz);
		}
	morton[t] = out;
}

__device__ __forceinline__ uint4 dilate1_x(const uint4 a) {
	uint4 r;
	r.x = a.x | (a.x << 1) | (a.x >> 1) | (a.y << 31);
	r.y = a.y | (a.y << 1) | (a.x >> 31) | (a.y >> 1) | (a.z << 31);
	r.z = a.z | (a.z << 1) | (a.y >> 31) | (a.z >> 1) | (a.w << 31);
	r.w = a.w | (a.w << 1) | (a.z >> 31) | (a.w >> 1);
	return r;
}

// (the plan travels as a kernel argument: its loops are wave-uniform, so the taps are scalar loads)
__global__ __launch_bounds__(256) void morph_rows_kernel(const MorphPlan plan, const uint4* __restrict__ in, uint4* __restrict__ out) {
	const uint32_t t = blockIdx.x * 256u + threadIdx.x; // row t: (z, y)
	const int32_t y = (int32_t)(t & 127u), z = (int32_t)(t >> 7);
	const uint32_t inv = plan.invert ? 0xffffffffu : 0u;
	uint4 acc = make_uint4(0, 0, 0, 0);
	int32_t h = plan.n_taps ? plan.half[0] : 0;
	for (uint32_t i = 0; i < plan.n_taps; ++i) {
		for (; h > plan.half[i]; --h) acc = dilate1_x(acc);
		const int32_t yy = y + plan.dy[i], zz = z + plan.dz[i];
		if (yy >= 0 && yy < (int32_t)kGrid && zz >= 0 && zz < (int32_t)kGrid) {
			const uint4 v = in[zz * (int32_t)kGrid + yy];
			acc.x |= v.x ^ inv; acc.y |= v.y ^ inv; acc.z |= v.z ^ inv; acc.w |= v.w ^ inv;
		}
	}
	for (; h > 0; --h) acc = dilate1_x(acc);
	out[t] = make_uint4(acc.x ^ inv, acc.y ^ inv, acc.z ^ inv, acc.w ^ inv);
}

__global__ __launch_bounds__(256) void selection_lattice_kernel(const uint32_t* __restrict__ rows, float4* __restrict__ lattice) {
	const uint32_t t = blockIdx.x * 256u + threadIdx.x; // lattice points 4 t .. 4 t + 3 of x + 128 y + 128^2 z
	const uint32_t i = 4u * t, x = i & 127u, y = (i >> 7) & 127u, z = i >> 14;
	uint32_t four = (rows[i >> 5] >> (i & 31u)) & 0xFu;
	if (y == 0u || y == kGrid - 1u || z == 0u || z == kGrid - 1u) four = 0u; // is_boundary cells stay out (growing_selection.cu:2126)
	if (x == 0u) four &= ~1u;
	if (x == kGrid - 4u) four &= ~8u;
	lattice[t] = make_float4((four & 1u) ? 1.f : 0.f, (four & 2u) ? 1.f : 0.f, (four & 4u) ? 1.f : 0.f, (four & 8u) ? 1.f : 0.f);
}

int launch_morph_pack(const uint32_t* d_morton_level, uint32_t* d_rows, void* stream) {
	hipLaunchKernelGGL(morph_pack_kernel, dim3(kMorphLevelWords / 256), dim3(256), 0, (hipStream_t)stream, d_morton_level, d_rows);
	NRS_LAUNCH_CHECK("morph_pack_kernel launch");
	return NRS_OK;
}
int launch_morph_unpack(const uint32_t* d_rows, uint32_t* d_morton_level, void* stream) {
	hipLaunchKernelGGL(morph_unpack_kernel, dim3(kMorphLevelWords / 256), dim3(256), 0, (hipStream_t)stream, d_rows, d_morton_level);
	NRS_LAUNCH_CHECK("morph_unpack_kernel launch");
	return NRS_OK;
}
int launch_morph_rows(const MorphPlan& plan, const uint32_t* d_rows_in, uint32_t* d_rows_out, void* stream) {
	if (plan.n_taps > kMorphMaxTaps) { snprintf(g_launch_err, sizeof(g_launch_err), "morph_rows_kernel: %u taps, at most %u", plan.n_taps, kMorphMaxTaps); return NRS_ERR_STATE; }
	hipLaunchKernelGGL(morph_rows_kernel, dim3(kGrid * kGrid / 256), dim3(256), 0, (hipStream_t)stream, plan, reinterpret_cast<const uint4*>(d_rows_in),
	                   reinterpret_cast<uint4*>(d_rows_out));
	NRS_LAUNCH_CHECK("morph_rows_kernel launch");
	return NRS_OK;
}
int launch_selection_lattice(const uint32_t* d_rows, float* d_lattice, void* stream) {
	hipLaunchKernelGGL(selection_lattice_kernel, dim3(kGridVol / 4 / 256), dim3(256), 0, (hipStream_t)stream, d_rows, reinterpret_cast<float4*>(d_lattice));
	NRS_LAUNCH_CHECK("selection_lattice_kernel launch");
	return NRS_OK;
}

} // namespace nrs
