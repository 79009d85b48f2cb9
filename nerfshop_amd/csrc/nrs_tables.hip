// nrs_tables.hip -- the builders of the tables the render kernel gathers from, and the operators on caller batches (gfx950).
//
//   cell_records_kernel  the cell-record cache of the coarse hash-grid levels (nrs_model_set_cell_cache).
//   weight_fragments_kernel, brick_*   the MFMA weight fragments read from HBM; the sparse cell records (nrs_model_set_sparse_cell_cache).
//   map_rays_kernel      EditOperator::map_rays / map_positions on caller batches.
#include <hip/hip_runtime.h>
#include "../../include/nrs.h"
#include "nrs_internal.h"
#include "nrs_launch.h"
#include "nrs_tables.h"
#include "nrs_vec.cuh"
#include "nrs_grid_math.cuh"
#include "nrs_edit_warp.cuh"

namespace nrs {

// ---------------------------------------------------------------------------------------------------------------
// Cell records (nrs_model_set_cell_cache): for every cell of a level, its 8 corner entries in corner order (x fastest),
// fetched with the level's own index function (grid.h:76-95 as restated in level_eval_slow) -- so a record gather returns
// exactly what the eight hashed / dense gathers would.  One thread per cell, 32 B written per thread, coalesced.
__global__ __launch_bounds__(256) void cell_records_kernel(const uint32_t* __restrict__ grid, const LevelParams lp, uint4* __restrict__ out) {
	const uint32_t n = lp.rec_res * lp.rec_res2;
	for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
		const uint32_t gx = i % lp.rec_res, gy = (i / lp.rec_res) % lp.rec_res, gz = i / lp.rec_res2;
		uint32_t v[8];
		#pragma unroll
		for (int c = 0; c < 8; ++c) {
			const uint32_t cx = gx + (c & 1), cy = gy + ((c >> 1) & 1), cz = gz + ((c >> 2) & 1);
			uint32_t index = lp.hashed ? ((cx * 1u) ^ (cy * 2654435761u) ^ (cz * 805459861u)) : (cx + cy * lp.resolution + cz * lp.res2);
			index %= lp.count;
			v[c] = grid[lp.offset + index];
		}
		uint4* o = out + 2 * ((size_t)lp.rec_first + i);
		o[0] = make_uint4(v[0], v[1], v[2], v[3]);
		o[1] = make_uint4(v[4], v[5], v[6], v[7]);
	}
}
int launch_cell_records(const DeviceModel& m, uint32_t n_levels, void* d_records, void* stream) {
	for (uint32_t l = 0; l < n_levels; ++l) {
		const LevelParams& lp = m.levels[l];
		const uint64_t n = (uint64_t)lp.rec_res * lp.rec_res2;
		const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + 255) / 256, 1u << 20);
		hipLaunchKernelGGL(cell_records_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, m.grid, lp, (uint4*)d_records);
	}
	return hipGetLastError() == hipSuccess ? NRS_OK : NRS_ERR_HIP;
}

// MFMA weight fragments from a parameter blob that lives on the device (nrs_model_set_params_device): frag[i] = params[src[i] - 1], or 0 where
// src[i] == 0 (padding rows).  src is make_weight_fragments' permutation, computed once per model on the host.
__global__ __launch_bounds__(256) void weight_fragments_kernel(const uint16_t* __restrict__ params, const uint16_t* __restrict__ src, uint16_t* __restrict__ frag, uint32_t n) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	const uint32_t k = src[i];
	// (kFragOne / kFragMinusOne: the constants of the selection fragments and of lowered networks; bit 15: a negated weight -- lower_weights, nrs_api_lowering.cpp)
	const uint32_t idx = k & (uint32_t)(kFragNegate - 1u);
	frag[i] = k == kFragOne ? (uint16_t)0x3C00 : (k == kFragMinusOne ? (uint16_t)0xBC00 : (idx ? (uint16_t)(params[idx - 1u] ^ (k & kFragNegate)) : (uint16_t)0));
}
int launch_weight_fragments(const uint16_t* d_params, const uint16_t* d_src, uint16_t* d_frag, uint32_t n, void* stream) {
	hipLaunchKernelGGL(weight_fragments_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_params, d_src, d_frag, n);
	NRS_LAUNCH_CHECK("weight_fragments_kernel launch");
	return NRS_OK;
}

// ---- sparse cell records (nrs_model_set_sparse_cell_cache) -------------------------------------------------------------------------
// brick_mark_kernel: one thread per cell of the 5-cascade mask (density-bitfield layout).  A marked cell allocates every 8^3-cell
// brick of the level that its box touches (one cell of margin: samples sit anywhere inside the density cell, borders included).
// Slots are handed out in arrival order; the records do not depend on it.
__global__ __launch_bounds__(256) void brick_mark_kernel(const LevelParams lp, const Box3 aabb, const uint8_t* __restrict__ mask, uint32_t* __restrict__ table,
                                                         uint32_t* __restrict__ counter, uint32_t* __restrict__ slots, uint32_t capacity) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= kGridVol * kCascades) return;
	if (!((mask[i >> 3] >> (i & 7u)) & 1u)) return;
	const uint32_t level = i / kGridVol, idx = i % kGridVol;
	const float s = ldexpf(1.0f, (int)level);
	const uint32_t cx = morton3D_invert(idx), cy = morton3D_invert(idx >> 1), cz = morton3D_invert(idx >> 2);
	const float c[3] = {(float)cx, (float)cy, (float)cz};
	int lo[3], hi[3];
	for (int k = 0; k < 3; ++k) {
		const float w0 = ((c[k] / (float)kGrid - 0.5f) * s + 0.5f - aabb.mn[k]) / (aabb.mx[k] - aabb.mn[k]);
		const float w1 = (((c[k] + 1.0f) / (float)kGrid - 0.5f) * s + 0.5f - aabb.mn[k]) / (aabb.mx[k] - aabb.mn[k]);
		if (w1 < 0.f || w0 > 1.f) return; // outside the scene box: no lookups there (records cover [0,1]^3)
		const int g0 = (int)floorf(fmaf(lp.scale, fmaxf(w0, 0.f), 0.5f)) - 1, g1 = (int)floorf(fmaf(lp.scale, fminf(w1, 1.f), 0.5f)) + 1;
		lo[k] = max(g0, 0) >> 3;
		hi[k] = min(g1, (int)lp.resolution - 1) >> 3;
	}
	for (int bz = lo[2]; bz <= hi[2]; ++bz)
		for (int by = lo[1]; by <= hi[1]; ++by)
			for (int bx = lo[0]; bx <= hi[0]; ++bx) {
				const uint32_t b = (uint32_t)bz * lp.rec_res2 + (uint32_t)by * lp.rec_res + (uint32_t)bx;
				if (table[b] != 0u) continue;
				if (atomicCAS(&table[b], 0u, 0xffffffffu) == 0u) {
					const uint32_t slot = atomicAdd(counter, 1u);
					if (slot < capacity) slots[slot] = b;
					__atomic_store_n(&table[b], slot + 1u, __ATOMIC_RELAXED);
				}
			}
}
// brick_fill_kernel: one thread per record of an allocated brick: the cell's 8 corner entries, fetched with the level's own index
// function exactly as cell_records_kernel does.
__global__ __launch_bounds__(256) void brick_fill_kernel(const uint32_t* __restrict__ grid, const LevelParams lp, const uint32_t* __restrict__ slots, uint32_t n_bricks,
                                                         uint4* __restrict__ out) {
	const uint64_t n = (uint64_t)n_bricks * kBrickCells;
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
		const uint32_t b = slots[i >> 9], within = (uint32_t)i & 511u; // (the thread's cell in x-fastest order; its record sits at brick_slot)
		const uint32_t bx = b % lp.rec_res, by = (b / lp.rec_res) % lp.rec_res, bz = b / lp.rec_res2;
		const uint32_t gx = bx * 8u + (within & 7u), gy = by * 8u + ((within >> 3) & 7u), gz = bz * 8u + (within >> 6);
		uint32_t v[8];
		#pragma unroll
		for (int c = 0; c < 8; ++c) {
			const uint32_t cx = gx + (c & 1), cy = gy + ((c >> 1) & 1), cz = gz + ((c >> 2) & 1);
			uint32_t index = lp.hashed ? ((cx * 1u) ^ (cy * 2654435761u) ^ (cz * 805459861u)) : (cx + cy * lp.resolution + cz * lp.res2);
			index %= lp.count;
			v[c] = grid[lp.offset + index];
		}
		uint4* o = out + 2 * ((size_t)lp.rec_first + (i & ~(uint64_t)511u) + brick_slot(within & 7u, (within >> 3) & 7u, within >> 6));
		o[0] = make_uint4(v[0], v[1], v[2], v[3]);
		o[1] = make_uint4(v[4], v[5], v[6], v[7]);
	}
}
int launch_brick_mark(const DeviceModel& m, const LevelParams& lp, const uint8_t* d_mask, uint32_t* d_table, uint32_t* d_counter, uint32_t* d_slots, uint32_t capacity, void* stream) {
	hipLaunchKernelGGL(brick_mark_kernel, dim3((kGridVol * kCascades + 255) / 256), dim3(256), 0, (hipStream_t)stream, lp, m.aabb, d_mask, d_table, d_counter, d_slots, capacity);
	NRS_LAUNCH_CHECK("brick_mark_kernel launch");
	return NRS_OK;
}
int launch_brick_fill(const DeviceModel& m, const LevelParams& lp, const uint32_t* d_slots, uint32_t n_bricks, void* d_records2, void* stream) {
	if (!n_bricks) return NRS_OK;
	const uint64_t n = (uint64_t)n_bricks * kBrickCells;
	const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + 255) / 256, 1u << 20);
	hipLaunchKernelGGL(brick_fill_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, m.grid, lp, d_slots, n_bricks, (uint4*)d_records2);
	NRS_LAUNCH_CHECK("brick_fill_kernel launch");
	return NRS_OK;
}

// ---- EditOperator::map_rays / map_positions on caller batches --------------------------------------------------------------
__global__ void map_rays_kernel(const DeviceEdit e, uint32_t n, float* __restrict__ coords, uint32_t ld, int with_dir, uint8_t* __restrict__ empty_mask) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	float* c = coords + (size_t)i * ld;
	f3 wpos = mk3(c[0], c[1], c[2]);
	f3 wdir = with_dir ? mk3(c[4], c[5], c[6]) : mk3(0.5f, 0.5f, 0.5f);
	const f3 p0 = wpos, d0 = wdir;
	const bool empty = edit_warp(e, with_dir != 0, wpos, wdir);
	if (wpos.x != p0.x || wpos.y != p0.y || wpos.z != p0.z) { c[0] = wpos.x; c[1] = wpos.y; c[2] = wpos.z; }
	if (with_dir && (wdir.x != d0.x || wdir.y != d0.y || wdir.z != d0.z)) { c[4] = wdir.x; c[5] = wdir.y; c[6] = wdir.z; }
	if (empty) empty_mask[i] = 1;
}

int launch_map_rays(const DeviceEdit& e, uint32_t n, float* d_coords, uint32_t ld, int with_dir, uint8_t* d_empty, void* stream) {
	if (n == 0) return NRS_OK;
	hipLaunchKernelGGL(map_rays_kernel, dim3((n + 127) / 128), dim3(128), 0, (hipStream_t)stream, e, n, d_coords, ld, with_dir, d_empty);
	NRS_LAUNCH_CHECK("map_rays_kernel launch");
	return NRS_OK;
}

} // namespace nrs
