// nrs_grid_math.cuh -- step, cascade and occupancy-grid arithmetic of a ray or a sample, and the warps between world and [0,1] coordinates.
//
// Everything here is plain fp32/u32 arithmetic whose operation ORDER is part of the contract: the file is
// compiled with -ffp-contract=off and the only fused multiply-adds are explicit fmaf(), so that the
// (t, dt, mip, cell) stream of every ray is bit-identical to the CPU oracle.  Citations are file:line in the
// reference checkout ("tn" = src/testbed_nerf.cu, "cn" = src/common_nerf.cu).
#pragma once
#include <hip/hip_runtime.h>
#include "nrs_internal.h"
#include "nrs_vec.cuh"

namespace nrs {

// ---- constants (common_nerf.h:16-39) ------------------------------------------------------------------------
#define NRS_SQRT3 1.73205080757f
#define NRS_MIN_STEP (NRS_SQRT3 / 1024)
#define NRS_MAX_STEP (NRS_MIN_STEP * (1 << (kCascades - 1)) * 1024 / kGrid)
#define NRS_NEAR_DISTANCE 0.05f

// ---- Morton (tcnn morton3D; x in the lowest bit) --------------------------------------------------------------
// (v * 0x00010001) & mask etc. of tcnn's expand_bits equals (v | v << s) & mask for v < 2^10: written with shifts because
// v_mul_lo_u32 is a quarter-rate instruction and this runs once per DDA step.
__device__ __forceinline__ uint32_t expand_bits(uint32_t v) {
	v = (v | (v << 16)) & 0xFF0000FFu;
	v = (v | (v << 8)) & 0x0F00F00Fu;
	v = (v | (v << 4)) & 0xC30C30C3u;
	v = (v | (v << 2)) & 0x49249249u;
	return v;
}
__device__ __forceinline__ uint32_t morton3D(uint32_t x, uint32_t y, uint32_t z) {
	return expand_bits(x) | (expand_bits(y) << 1) | (expand_bits(z) << 2);
}
__device__ __forceinline__ uint32_t morton3D_invert(uint32_t x) {
	x = x & 0x49249249u;
	x = (x | (x >> 2)) & 0xc30c30c3u;
	x = (x | (x >> 4)) & 0x0f00f00fu;
	x = (x | (x >> 8)) & 0xff0000ffu;
	x = (x | (x >> 16)) & 0x0000ffffu;
	return x;
}

// ---- step / grid math (cn:80-177) -------------------------------------------------------------------------------
// clamp(t * cone, MIN, MAX) as one v_med3_f32: the median of (v, lo, hi) is the clamp for every non-NaN v (t * cone >= 0)
__device__ __forceinline__ float calc_dt(float t, float cone_angle) { return __builtin_amdgcn_fmed3f(t * cone_angle, NRS_MIN_STEP, NRS_MAX_STEP); }

// frexpf's exponent: x = m * 2^e, 0.5 <= |m| < 1; 0 for x == 0
__device__ __forceinline__ int frexp_exponent(float x) {
	uint32_t u = __float_as_uint(x) & 0x7fffffffu;
	if (u == 0) return 0;
	uint32_t ef = u >> 23;
	if (ef == 0) return -117 - __clz((int)u);
	return (int)ef - 126;
}
// res is a power of two (128 >> mip): dividing by it equals multiplying by inv_res = 1/res exactly, bit for bit
__device__ __forceinline__ float distance_to_next_voxel(f3 pos, f3 dir, f3 idir, uint32_t res, float inv_res) {
	f3 p = (float)res * pos;
	float tx = (floorf(p.x + 0.5f + 0.5f * signf_(dir.x)) - p.x) * idir.x;
	float ty = (floorf(p.y + 0.5f + 0.5f * signf_(dir.y)) - p.y) * idir.y;
	float tz = (floorf(p.z + 0.5f + 0.5f * signf_(dir.z)) - p.z) * idir.z;
	float t = fminf(fminf(tx, ty), tz);
	return fmaxf(t * inv_res, 0.0f);
}
__device__ __forceinline__ float advance_to_next_voxel(float t, float cone_angle, f3 pos, f3 dir, f3 idir, uint32_t res, float inv_res) {
	float t_target = t + distance_to_next_voxel(pos, dir, idir, res, inv_res);
	if (cone_angle == 0.f) {
		// constant step (aabb_scale 1): the same chain of float additions as the loop below, but the first eight are
		// straight-line select code -- a cell diagonal is at most sqrt(3)/128 = 8 steps of sqrt(3)/1024, so the divergent
		// loop (whose trip count is the wave's maximum) only runs for coarser cascades.
		// t += (t < t_target) ? dt : 0 without a compare/select pair (VCC hazards): m = clamp((t_target - t) * 2^100, 0, 1)
		// is exactly 1 or 0, and fmaf(m, dt, t) rounds t + dt exactly as the addition does (m * dt is exact).
		t += NRS_MIN_STEP;
		#pragma unroll
		for (int k = 0; k < 7; ++k) {
			const float m = __builtin_amdgcn_fmed3f((t_target - t) * 0x1p100f, 0.0f, 1.0f);
			t = fmaf(m, NRS_MIN_STEP, t);
		}
		while (t < t_target) t += NRS_MIN_STEP;
		return t;
	}
	do {
		t += calc_dt(t, cone_angle);
	} while (t < t_target);
	return t;
}
__device__ __forceinline__ uint32_t cascaded_grid_idx_at(f3 pos, uint32_t mip) {
	float mip_scale = ldexpf(1.0f, -(int)mip);
	pos = pos - mk3(0.5f, 0.5f, 0.5f);
	pos = pos * mip_scale;
	pos = pos + mk3(0.5f, 0.5f, 0.5f);
	int ix = (int)(pos.x * (float)kGrid), iy = (int)(pos.y * (float)kGrid), iz = (int)(pos.z * (float)kGrid);
	return morton3D((uint32_t)clampi_(ix, 0, kGrid - 1), (uint32_t)clampi_(iy, 0, kGrid - 1), (uint32_t)clampi_(iz, 0, kGrid - 1));
}
__device__ __forceinline__ bool get_bitfield_at(uint32_t cell_idx, uint32_t level, const uint8_t* __restrict__ bitfield) {
	return bitfield[cell_idx / 8 + (kGridVol * level) / 8] & (1 << (cell_idx % 8));
}
__device__ __forceinline__ bool density_grid_occupied_at(f3 pos, const uint8_t* __restrict__ bitfield, uint32_t mip) {
	return get_bitfield_at(cascaded_grid_idx_at(pos, mip), mip, bitfield);
}
// min(4, max(0, frexp_exponent(maxval) + 1)) without branches: the biased exponent alone decides (sub-normal maxval
// clamps to 0 like every maxval < 0.5), except frexpf(0) = 0 * 2^0, which the reference turns into mip 1.
__device__ __forceinline__ int mip_from_pos(f3 pos) {
	float maxval = fmaxf(fmaxf(fabsf(pos.x - 0.5f), fabsf(pos.y - 0.5f)), fabsf(pos.z - 0.5f));
	const uint32_t u = __float_as_uint(maxval); // maxval >= 0
	const int mip = min((int)kCascades - 1, max(0, (int)(u >> 23) - 125));
	return u == 0 ? 1 : mip;
}
__device__ __forceinline__ int mip_from_dt(float dt, f3 pos) {
	int mip = mip_from_pos(pos);
	dt *= 2 * kGrid;
	// dt >= 1 is a normal number: frexp exponent = biased exponent - 126; for dt < 1 that is <= 0 <= mip, so max() keeps mip
	const int exponent = (int)(__float_as_uint(dt) >> 23) - 126;
	return min((int)kCascades - 1, max(exponent, mip));
}
__device__ __forceinline__ f3 warp_position(f3 pos, const Box3& aabb) {
	return {(pos.x - aabb.mn[0]) / (aabb.mx[0] - aabb.mn[0]), (pos.y - aabb.mn[1]) / (aabb.mx[1] - aabb.mn[1]),
	        (pos.z - aabb.mn[2]) / (aabb.mx[2] - aabb.mn[2])};
}
__device__ __forceinline__ f3 unwarp_position(f3 pos, const Box3& aabb) {
	return {aabb.mn[0] + pos.x * (aabb.mx[0] - aabb.mn[0]), aabb.mn[1] + pos.y * (aabb.mx[1] - aabb.mn[1]),
	        aabb.mn[2] + pos.z * (aabb.mx[2] - aabb.mn[2])};
}
__device__ __forceinline__ f3 warp_direction(f3 d) { return {(d.x + 1.0f) * 0.5f, (d.y + 1.0f) * 0.5f, (d.z + 1.0f) * 0.5f}; }
__device__ __forceinline__ f3 unwarp_direction(f3 d) { return {d.x * 2.0f - 1.0f, d.y * 2.0f - 1.0f, d.z * 2.0f - 1.0f}; }
__device__ __forceinline__ float warp_dt(float dt) {
	float max_stepsize = NRS_MIN_STEP * (1 << (kCascades - 1));
	return (dt - NRS_MIN_STEP) / (max_stepsize - NRS_MIN_STEP);
}
__device__ __forceinline__ float unwarp_dt(float dt) {
	float max_stepsize = NRS_MIN_STEP * (1 << (kCascades - 1));
	return dt * (max_stepsize - NRS_MIN_STEP) + NRS_MIN_STEP;
}

__device__ __forceinline__ void ray_intersect(const float* mn, const float* mx, f3 pos, f3 dir, float& tmin_out) {
	const float FMAX = 3.402823466e+38f;
	float tmin = (mn[0] - pos.x) / dir.x, tmax = (mx[0] - pos.x) / dir.x;
	if (tmin > tmax) { float s = tmin; tmin = tmax; tmax = s; }
	float tymin = (mn[1] - pos.y) / dir.y, tymax = (mx[1] - pos.y) / dir.y;
	if (tymin > tymax) { float s = tymin; tymin = tymax; tymax = s; }
	if (tmin > tymax || tymin > tmax) { tmin_out = FMAX; return; }
	if (tymin > tmin) tmin = tymin;
	if (tymax < tmax) tmax = tymax;
	float tzmin = (mn[2] - pos.z) / dir.z, tzmax = (mx[2] - pos.z) / dir.z;
	if (tzmin > tzmax) { float s = tzmin; tzmin = tzmax; tzmax = s; }
	if (tmin > tzmax || tzmin > tmax) { tmin_out = FMAX; return; }
	if (tzmin > tmin) tmin = tzmin;
	tmin_out = tmin;
}

} // namespace nrs
