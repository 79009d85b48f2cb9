// nrs_march.cuh -- the walk of a ray through the occupancy grid to its next occupied cell, with its result-preserving shortcuts:
// the occupied bounds, the look-ahead mask, the lattice jump.  Citations as in nrs_grid_math.cuh.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/nrs.h"
#include "nrs_internal.h"
#include "nrs_vec.cuh"
#include "nrs_grid_math.cuh"
#include "nrs_random.cuh"
#include "nrs_camera.cuh"

namespace nrs {

// Does the ray o + d*s, s >= t, still meet the box?  (slab test; NaNs from 0 * inf drop out of fminf / fmaxf)
__device__ __forceinline__ bool ray_meets_box_ahead(const Box3& b, f3 o, f3 idir, float t) {
	const float ax = (b.mn[0] - o.x) * idir.x, bx = (b.mx[0] - o.x) * idir.x;
	const float ay = (b.mn[1] - o.y) * idir.y, by = (b.mx[1] - o.y) * idir.y;
	const float az = (b.mn[2] - o.z) * idir.z, bz = (b.mx[2] - o.z) * idir.z;
	const float tnear = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz), t));
	const float tfar = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
	return tnear <= tfar;
}

// Marching shortcut 2 (result-preserving).  kCoarse^3 blocks over occ_box carry "some occupied cell (any cascade,
// inflated like occ_box) overlaps this block".  coarse_safe_until walks the blocks along o + d*s, s >= t (Amanatides-Woo,
// <= 3 * kCoarse - 2 steps) and returns the parameter up to which the ray provably meets no occupied cell:
//   < 0       nothing ahead at all: no further sample can be emitted, the caller retires the ray at once;
//   otherwise the entry into the first marked block, minus a margin that dwarfs the walk's float error.
// `mask` is the LDS copy of DeviceModel::coarse_mask.
__device__ __forceinline__ float coarse_safe_until(const DeviceModel& m, const uint32_t* __restrict__ mask, f3 o, f3 d, f3 idir, float t) {
	const Box3& b = m.occ.box;
	const float ax = (b.mn[0] - o.x) * idir.x, bx = (b.mx[0] - o.x) * idir.x;
	const float ay = (b.mn[1] - o.y) * idir.y, by = (b.mx[1] - o.y) * idir.y;
	const float az = (b.mn[2] - o.z) * idir.z, bz = (b.mx[2] - o.z) * idir.z;
	const float tnear = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz), t));
	const float tfar = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
	if (!(tnear <= tfar)) return -1.f;
	const f3 p = o + d * tnear;
	const float hi = (float)(kCoarse - 1);
	int cx = (int)__builtin_amdgcn_fmed3f((p.x - b.mn[0]) * m.occ.inv_cell[0], 0.f, hi);
	int cy = (int)__builtin_amdgcn_fmed3f((p.y - b.mn[1]) * m.occ.inv_cell[1], 0.f, hi);
	int cz = (int)__builtin_amdgcn_fmed3f((p.z - b.mn[2]) * m.occ.inv_cell[2], 0.f, hi);
	const int sx = d.x >= 0.f ? 1 : -1, sy = d.y >= 0.f ? 1 : -1, sz = d.z >= 0.f ? 1 : -1;
	const float inf = __builtin_huge_valf();
	float tmx = d.x != 0.f ? ((b.mn[0] + (float)(cx + (sx > 0 ? 1 : 0)) * m.occ.cell[0]) - o.x) * idir.x : inf;
	float tmy = d.y != 0.f ? ((b.mn[1] + (float)(cy + (sy > 0 ? 1 : 0)) * m.occ.cell[1]) - o.y) * idir.y : inf;
	float tmz = d.z != 0.f ? ((b.mn[2] + (float)(cz + (sz > 0 ? 1 : 0)) * m.occ.cell[2]) - o.z) * idir.z : inf;
	const float tdx = fabsf(m.occ.cell[0] * idir.x), tdy = fabsf(m.occ.cell[1] * idir.y), tdz = fabsf(m.occ.cell[2] * idir.z);
	float t_enter = tnear; // parameter at which the current block was entered
	#pragma unroll 1
	for (int it = 0; it < (int)(3 * kCoarse); ++it) {
		const uint32_t idx = ((uint32_t)cz * kCoarse + (uint32_t)cy) * kCoarse + (uint32_t)cx;
		if ((mask[idx >> 5] >> (idx & 31)) & 1u) return fmaxf(t_enter - 1e-4f, 0.f);
		const bool step_x = tmx <= tmy && tmx <= tmz, step_y = !step_x && tmy <= tmz, step_z = !step_x && !step_y;
		t_enter = step_x ? tmx : (step_y ? tmy : tmz);
		cx += step_x ? sx : 0; cy += step_y ? sy : 0; cz += step_z ? sz : 0;
		tmx += step_x ? tdx : 0.f; tmy += step_y ? tdy : 0.f; tmz += step_z ? tdz : 0.f;
		if ((uint32_t)(cx | cy | cz) > kCoarse - 1) return -1.f; // left the box through an empty block (negative indices have high bits set)
	}
	return 0.f; // unreachable (a ray crosses at most 3 * kCoarse - 2 blocks); "nothing is known" keeps the plain walk
}

// ---- the lean walk in O(1) (round 5) ----------------------------------------------------------------------------------------------------------------
// With a constant step (cone_angle == 0: dt = MIN_STEP everywhere) every parameter the walk ever stands on is a LATTICE point t_0 (+) dt (+) dt ... -- the same
// chain of float additions whatever the cells are; the cells only decide at which lattice points the walk STOPS (the first lattice point at or behind each cell
// border: advance_to_next_voxel).  Inside one binade [2^e, 2^(e+1)) the rounded addition t (+) dt adds a CONSTANT number q of ulps (dt = (I + f) ulp(t), f != 1/2:
// q = I + (f > 1/2) -- no ties, so no dependence on the parity of t), so the lattice point k steps on is the integer addition bits(t) + k q: no chain needed.
// What the chain-free jump cannot know is at which lattice points the walk stopped on the way -- and over a stretch that is known to be empty (t < t_safe,
// coarse_safe_until) it does not need to, with one exception: the walk must continue from a lattice point at which the reference's walk STOPS, because the border
// parameter t + distance_to_next_voxel(pos(t)) carries the rounding of the stop it is computed from.  So: jump to a lattice point t_k a cell and a half short of
// t_safe, take ONE ordinary step of the walk from there to u = the first lattice point behind the border g of t_k's cell, and accept u only if no lattice point
// lies within +-B of g, where B bounds the difference between the border parameters computed from any two lattice points of one cell (derivation: DESIGN.md 4,
// "lattice jump": |g - exact border| <= (1.2e-7 t + 6e-8) |1/d_axis| + 1.2e-7 t; B is ten times that).  Then every evaluation of that border -- the reference's,
// from its own stop in that cell, included -- selects the same u: u IS the reference's next stop, and the walk goes on from it bit for bit.  If a lattice point
// sits inside the band (about 1 % of the jumps), or anything else is unusual (a tie, a sub-normal, the stretch leaves the unit cube where the cascade could
// change), the function declines and the ordinary lean walk runs.  The (t, dt) streams stay bit-identical to the oracle's cell-by-cell walk (tests/test_gpu_parity.py).
constexpr uint32_t kJumpMinSteps = 14u; // (a cell is 4.6 steps; the jump costs about two cells of lean walk)
__device__ __forceinline__ bool lattice_jump(f3 o, f3 d, f3 idir, float t_safe, uint32_t mip, float& t) {
	// (Straight-line: every condition is folded into one predicate and the candidate is computed whether or not it will be taken -- nested early exits cost this
	// kernel scalar registers for the saved execution masks.  And written with VOP2-encodable literals: a literal operand of a three-source instruction needs a
	// register on gfx9, which the compiler hoists out of the frame loop -- a dozen such constants once pushed the kernel past its 128 registers.)
	const float margin = 0.02f * (float)(1u << mip); // a cell diagonal (1.35e-2 at cascade 0) + two steps + slack
	const float k_want = floorf((t_safe - t - margin) * (1.0f / NRS_MIN_STEP)); // lattice steps to take (a lattice increment differs from dt by < ulp(t) / 2: 1e-5 over a stretch)
	bool ok = k_want >= (float)kJumpMinSteps && k_want < 60000.0f; // (false for a NaN)
	float k_left = ok ? k_want : 0.0f;
	float tc = t;
	// Two binade segments with three ordinary additions behind each: a stretch of the lego-like scenes starts below t = 1 and ends above it, and a jump that stopped
	// at the binade's end would leave the rest to the cell-by-cell walk of the slowest lane.  (The additions are lattice steps like any other.)
	#pragma unroll 1
	for (int seg = 0; seg < 2; ++seg) {
		const uint32_t b = __float_as_uint(tc);
		const int e_t = (int)(b >> 23); // tc > 0: the sign bit is clear
		// dt in ulps of this binade: x = dt 2^(150 - e_t), exact (a power of two); the lattice increment is x rounded to an integer, a constant as long as x is not
		// half-way between two (round-to-even would then look at the parity of t): such a binade -- or one out of range -- is not jumped through
		const float x = ldexpf(NRS_MIN_STEP, 150 - e_t), qf = rintf(x);
		const bool seg_ok = e_t >= 24 && e_t <= 137 && fabsf(x - qf) != 0.5f && qf >= 1.0f && qf < 8388608.0f; // (e_t <= 137: ulp(t) <= 2^-9 < dt)
		const float left = (float)(0x7fffffu - (b & 0x7fffffu)); // ulps to the binade's last value
		const float k_bin = fmaxf(floorf(left * __builtin_amdgcn_rcpf(qf)) - 1.0f, 0.0f); // lattice points left in the binade (rounded down with room)
		const float k = seg_ok ? fminf(k_left, k_bin) : 0.0f;
		tc = __uint_as_float(b + (uint32_t)k * (uint32_t)qf);
		k_left -= k;
		#pragma unroll
		for (int i = 0; i < 3; ++i) {
			const bool step = k_left > 0.0f;
			tc = step ? tc + NRS_MIN_STEP : tc;
			k_left = step ? k_left - 1.0f : k_left;
		}
	}
	ok = ok && (k_want - k_left) >= (float)kJumpMinSteps + 8.0f;
	// the cascade must be the same at every stop on the way: both ends strictly inside the unit cube, where mip_from_pos is 0 (cone_angle == 0: mip_from_dt adds nothing)
	ok = ok && mip_from_pos(o + d * t) == 0 && mip_from_pos(o + d * tc) == 0;
	__builtin_amdgcn_sched_barrier(0); // (stage by stage: interleaved, the stages' temporaries add up)
	// Up to three candidates: the lattice point reached, then the ones 4 and 8 steps before it (integer subtraction inside the binade: the same lattice).  A candidate
	// that fails the band test below would fail it again on every later attempt from this walk -- the attempts all aim at the same lattice point -- and ONE lane per
	// packet walking its stretch cell by cell is what the whole wave then waits for (measured: 36 instead of 9 wave trips per packet).
	const uint32_t bk = __float_as_uint(tc);
	const float q_here = rintf(ldexpf(NRS_MIN_STEP, 150 - (int)(bk >> 23)));
	const uint32_t back = 4u * (uint32_t)q_here;
	const uint32_t res = kGrid >> mip;
	const float inv_res = ldexpf(1.0f, (int)mip - 7);
	const float B = (fmaxf(fmaxf(fabsf(idir.x), fabsf(idir.y)), fabsf(idir.z)) + 1.0f) * 2e-6f * fmaxf(t_safe, 1.0f);
	bool taken = false;
	float t_new = t;
	#pragma unroll 1
	for (uint32_t attempt = 0; attempt < 3u; ++attempt) {
		//  a back-off candidate needs one full increment of room above the binade's start: the first lattice point of a binade can sit q ulps above 2^e,
		// and bk - 4q could then land ON 2^e, which is not on the lattice
		const bool in_binade = attempt == 0u || (bk & 0x7fffffu) >= attempt * back + (uint32_t)q_here;
		const float tk = __uint_as_float(bk - (in_binade ? attempt * back : 0u));
		const f3 pk = o + d * tk;
		const float g = tk + distance_to_next_voxel(pk, d, idir, res, inv_res);
		// one ordinary step of the walk from t_k (advance_to_next_voxel's constant-step chain; the candidate's own while-loop tail cannot run: a cell of the unit cube's
		// cascade is at most 8 steps, and for coarser cells -- min_mip > 0 -- the predicate below declines when the eight steps did not reach the border)
		float u = tk + NRS_MIN_STEP;
		#pragma unroll
		for (int i = 0; i < 7; ++i) {
			const float mstep = __builtin_amdgcn_fmed3f((g - u) * 0x1p100f, 0.0f, 1.0f);
			u = fmaf(mstep, NRS_MIN_STEP, u);
		}
		bool pass = ok && in_binade && u >= g;
		pass = pass && (g + NRS_MIN_STEP + B < t_safe);             // the lean walk's own hand-over test at the stop in t_k's cell, band included
		pass = pass && (u - g > B) && (g - (u - NRS_MIN_STEP) > B); // no lattice point inside the band (also false for a non-finite B: axis-parallel rays)
		t_new = (pass && !taken) ? u : t_new;
		taken = taken || pass;
		if (!__any(ok && !taken)) break; // (wave-uniform: every lane that can jump has its stop)
	}
	t = t_new;
	return taken;
}

// The inner loop shared by advance_pos_nerf (tn:589-603) and generate_next_nerf_network_inputs (tn:668-692):
// advance t until the ray sits in an occupied cell (returns true; pos/dt valid) or leaves the render box (false).
//
// Shortcut 1: occ_box bounds all occupied cells of all cascades (inflated).  Outside it every occupancy test of the
// reference is false, so (i) the bitfield lookup is skipped -- the DDA recurrence that decides WHICH t values get tested is
// still executed verbatim, so the first accepted t is bit-identical -- and (ii) once the remaining ray cannot meet the box
// any more, no further sample can ever be emitted and the walk to the far side of the render box is cut short.
//
// Shortcut 2: when the cell the ray stands in is empty, the coarse mask is consulted ONCE (coarse_safe_until).  Rays with
// nothing ahead are retired.  For the others the stretch up to t_safe is walked by the LEAN loop below: the same float
// operations on t in the same order (position, cascade, distance to the voxel border, the chain of step additions) but
// none of the tests whose outcome is known there -- inside the render box (t_safe is clipped to it), cell empty.  The
// lean loop hands over BEFORE a step could land beyond t_safe; the full loop then re-enters at a t it would have reached
// itself, so the (t, dt) stream stays bit-identical (tests/test_gpu_parity.py compares it against the oracle).
// The look-ahead of shortcut 2 is repeated every kLookEvery empty cells of a walk, not only at its first: a ray that leaves
// the object through blocks that are marked (they touch the surface) but empty along its path used to walk on, cell by cell
// with a full test each, until it left the occupied bounds; a few cells on, nothing is marked ahead any more and it can be
// retired at once (or lean-walked to the next marked block).  Measured (Gsamples/s, lego + cage edit; ms for a 64x40-pixel
// frame): once per walk 9.0 / 0.84, every 3rd cell 9.43 / 0.58, 6th 9.92 / 0.56, 10th 9.80 / 0.55, 16th 9.82 / 0.58, 32nd 9.54 / 0.65.
constexpr float kJumpSpan = 0.06f; // remaining stretch from which the lattice jump is attempted (22 steps + the margin: nothing to gain below; 0.04 / 0.10 measured the same)
constexpr int kLookEvery = 6;
// The Morton code of an occupancy cell from a 128-entry table in LDS (spread3(v) = the bits of v at every third position; staged
// behind the look-ahead mask by stage_march_lds) -- three ds_read + two v_lshl_or instead of 28 VALU instructions per occupancy test; the cell index
// and therefore every decision stay the same.
constexpr uint32_t kMarchLdsWords = kCoarseWords + kGrid; // look-ahead mask | spread3 table
__device__ __forceinline__ void stage_march_lds(uint32_t* __restrict__ lds, const uint32_t* __restrict__ mask) { // (the caller's barrier publishes it)
	for (uint32_t i = threadIdx.x; i < kCoarseWords; i += blockDim.x) lds[i] = mask[i];
	for (uint32_t i = threadIdx.x; i < kGrid; i += blockDim.x) lds[kCoarseWords + i] = expand_bits(i);
}
// The voxel walk keeps the 64-bit word of the bitfield it last read -- in Morton order that is one 4 x 4 x 4 block of cells of one
// cascade -- and a test that falls into the same block is answered from the registers.  A ray that walks through empty cells next to the surface (the
// silhouette rays that bound small launches: DESIGN 5) then pays the bitfield's load latency once per block instead of once per cell; when no lane of
// the wave needs a new word the load is skipped altogether.  Pure caching: the decisions are the bitfield's.
struct OccWord { uint32_t tag; uint32_t lo, hi; };
// bit number of the cell of cascade `mip` that holds pos, in the concatenated bitfield (cn:117-141 through the LDS spread table)
__device__ __forceinline__ uint32_t occupancy_bit_index(f3 pos, uint32_t mip, const uint32_t* __restrict__ march_lds) {
	const float mip_scale = ldexpf(1.0f, -(int)mip);
	f3 q = pos - mk3(0.5f, 0.5f, 0.5f);
	q = q * mip_scale;
	q = q + mk3(0.5f, 0.5f, 0.5f);
	const int ix = (int)(q.x * (float)kGrid), iy = (int)(q.y * (float)kGrid), iz = (int)(q.z * (float)kGrid);
	const uint32_t* spread = march_lds + kCoarseWords;
	return (spread[clampi_(ix, 0, kGrid - 1)] | (spread[clampi_(iy, 0, kGrid - 1)] << 1) | (spread[clampi_(iz, 0, kGrid - 1)] << 2)) + mip * kGridVol;
}
__device__ __forceinline__ bool occupied_at_cached(f3 pos, const uint8_t* __restrict__ bitfield, uint32_t mip, const uint32_t* __restrict__ march_lds, OccWord& w) {
	const uint32_t idx = occupancy_bit_index(pos, mip, march_lds);
	const uint32_t tag = idx >> 6;
	if (tag != w.tag) {
		const uint2 v = reinterpret_cast<const uint2*>(bitfield)[tag];
		w.tag = tag; w.lo = v.x; w.hi = v.y;
	}
	const uint32_t bit = idx & 63u;
	return (((bit & 32u) ? w.hi : w.lo) >> (bit & 31u)) & 1u;
}
__device__ __forceinline__ bool occupied_at(f3 pos, const uint8_t* __restrict__ bitfield, uint32_t mip, const uint32_t* __restrict__ march_lds) {
	const float mip_scale = ldexpf(1.0f, -(int)mip);
	f3 q = pos - mk3(0.5f, 0.5f, 0.5f);
	q = q * mip_scale;
	q = q + mk3(0.5f, 0.5f, 0.5f);
	const int ix = (int)(q.x * (float)kGrid), iy = (int)(q.y * (float)kGrid), iz = (int)(q.z * (float)kGrid);
	const uint32_t* spread = march_lds + kCoarseWords;
	const uint32_t idx = spread[clampi_(ix, 0, kGrid - 1)] | (spread[clampi_(iy, 0, kGrid - 1)] << 1) | (spread[clampi_(iz, 0, kGrid - 1)] << 2);
	return get_bitfield_at(idx, mip, bitfield);
}
// 1 / d (three IEEE divisions, ~40 issue slots) is only needed once the ray stands in an EMPTY cell; the common call -- the next
// sample of a ray inside the object -- finds an occupied cell at once.  The first test is peeled off in front of the loop, the reciprocal formed behind it.
// JUMP: compile lattice_jump into this instance (the two hot ones: the fill's first_hit and the per-round walk of one-lane rounds; the team walks keep the plain lean
// walk -- every inlined copy costs scalar registers in a kernel that spills them)
template <bool JUMP = false>
__device__ __forceinline__ bool march_to_occupied(const nrs_render_params& p, const DeviceModel& m, const uint32_t* __restrict__ march_lds, f3 o, f3 d,
                                                  float& t, f3& pos, float& dt, uint32_t* n_iter = nullptr) {
	const uint32_t* __restrict__ coarse_mask = march_lds;
	const uint8_t* __restrict__ bitfield = m.bitfield;
	const Box3& occ_box = m.occ.box;
	Box3 bb;
	#pragma unroll
	for (int i = 0; i < 3; ++i) { bb.mn[i] = p.render_aabb_min[i]; bb.mx[i] = p.render_aabb_max[i]; }
	const float cone = p.cone_angle_constant;
	int until_look = 0; // trips until the next look-ahead
	uint32_t mip;
	bool in_occ;
	OccWord occ_word{0xffffffffu, 0u, 0u};
	#define NRS_OCCUPIED(pos_, mip_) occupied_at_cached(pos_, bitfield, mip_, march_lds, occ_word)
	if (n_iter) ++*n_iter; // profiling build only
	pos = o + d * t;
	if (!box_contains(bb, pos)) return false;
	dt = calc_dt(t, cone);
	mip = max(p.min_mip, (uint32_t)mip_from_dt(dt, pos));
	in_occ = box_contains(occ_box, pos);
	if (in_occ && NRS_OCCUPIED(pos, mip)) return true;
	const f3 idir = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
	bool first = true;
	while (1) {
		if (!first) {
			if (n_iter) ++*n_iter; // profiling build only
			pos = o + d * t;
			if (!box_contains(bb, pos)) return false;
			dt = calc_dt(t, cone);
			mip = max(p.min_mip, (uint32_t)mip_from_dt(dt, pos));
			in_occ = box_contains(occ_box, pos);
			if (in_occ && NRS_OCCUPIED(pos, mip)) return true;
		}
		first = false;
		if (!in_occ && !ray_meets_box_ahead(occ_box, o, idir, t)) return false;
		if (until_look-- == 0) {
			until_look = kLookEvery;
			float t_safe = coarse_safe_until(m, coarse_mask, o, d, idir, t);
			if (t_safe < 0.f) return false;
			{ // clip to the exit of the render box: the lean loop carries no containment test
				const float ax = (bb.mn[0] - o.x) * idir.x, bx = (bb.mx[0] - o.x) * idir.x;
				const float ay = (bb.mn[1] - o.y) * idir.y, by = (bb.mx[1] - o.y) * idir.y;
				const float az = (bb.mn[2] - o.z) * idir.z, bz = (bb.mx[2] - o.z) * idir.z;
				t_safe = fminf(t_safe, fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz)) - 1e-4f);
			}
			// lean walk: every position it stands on has parameter < t_safe
			while (1) {
				// (tried in EVERY pass of the lean walk, not once in front of it: a lane that declines -- a lattice point in the guard band, the end of a binade, the
				// entry point on the cube's face -- takes one ordinary step and tries again from there; a wave is as slow as its slowest lane, and one lane in a
				// hundred walking the whole stretch cell by cell would keep most waves waiting)
				if (JUMP && cone == 0.f && t_safe - t > kJumpSpan && lattice_jump(o, d, idir, t_safe, mip, t)) {
					if (n_iter) ++*n_iter;
					pos = o + d * t;
					dt = calc_dt(t, cone);
					mip = max(p.min_mip, (uint32_t)mip_from_dt(dt, pos));
				}
				const uint32_t lres = kGrid >> mip;
				const float linv = ldexpf(1.0f, (int)mip - 7);
				// one step past the border is the farthest the next position can be (first lattice point >= the border)
				const float border = t + distance_to_next_voxel(pos, d, idir, lres, linv);
				if (!(border + calc_dt(border, cone) < t_safe)) break;
				t = advance_to_next_voxel(t, cone, pos, d, idir, lres, linv);
				if (n_iter) ++*n_iter;
				pos = o + d * t;
				dt = calc_dt(t, cone);
				mip = max(p.min_mip, (uint32_t)mip_from_dt(dt, pos));
			}
		}
		uint32_t res = kGrid >> mip;
		t = advance_to_next_voxel(t, cone, pos, d, idir, res, ldexpf(1.0f, (int)mip - 7));
	}
	#undef NRS_OCCUPIED
}

// march_to_occupied's first test on its own: true when the walk from parameter t would return at once (inside the render box, in an occupied cell)
__device__ __forceinline__ bool stands_in_occupied_cell(const nrs_render_params& p, const DeviceModel& m, const uint32_t* __restrict__ march_lds, f3 o, f3 d, float t) {
	Box3 bb;
	#pragma unroll
	for (int i = 0; i < 3; ++i) { bb.mn[i] = p.render_aabb_min[i]; bb.mx[i] = p.render_aabb_max[i]; }
	const f3 pos = o + d * t;
	if (!box_contains(bb, pos)) return false;
	const float dt = calc_dt(t, p.cone_angle_constant);
	const uint32_t mip = max(p.min_mip, (uint32_t)mip_from_dt(dt, pos));
	if (!box_contains(m.occ.box, pos)) return false;
	return occupied_at(pos, m.bitfield, mip, march_lds);
}

// advance_pos_nerf, tn:557-606: jitter by one Sobol value, then skip to the first occupied cell
template <bool SPP = false>
__device__ __forceinline__ bool first_hit(const nrs_render_params& p, const DeviceModel& m, const uint32_t* __restrict__ march_lds, uint32_t pixel_idx, Ray& r,
                                          uint32_t* n_iter = nullptr, uint32_t spp = 0u) {
	float dt = calc_dt(r.t, p.cone_angle_constant);
	r.t += ld_random_val(SPP ? spp : p.spp_index, pixel_idx * 786433u) * dt;
	f3 pos;
	return march_to_occupied<true>(p, m, march_lds, r.o, r.d, r.t, pos, dt, n_iter);
}

} // namespace nrs
