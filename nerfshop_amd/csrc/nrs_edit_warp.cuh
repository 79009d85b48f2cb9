// nrs_edit_warp.cuh -- the edit operators as a sample meets them: the tet search and the cage warp, the affine duplication,
// the membrane (Poisson) residual.  Citations as in nrs_grid_math.cuh.
#pragma once
#include <hip/hip_runtime.h>
#include "nrs_internal.h"
#include "nrs_cage.h"
#include "nrs_vec.cuh"
#include "nrs_grid_math.cuh"
#include "nrs_march.cuh"

namespace nrs {

// ---- tet warp: selection_utils.h:10-47, cage_deformation.cu:136-269 -----------------------------------------------
__device__ __forceinline__ float scalar_tp(f3 a, f3 b, f3 c) { return dot3(a, cross3(b, c)); }
__device__ __forceinline__ bool same_side_tet(f3 v1, f3 v2, f3 v3, f3 v4, f3 p) {
	f3 normal = cross3(v2 - v1, v3 - v1);
	float dotV4 = dot3(normal, v4 - v1);
	float dotP = dot3(normal, p - v1);
	return signbit(dotV4) == signbit(dotP);
}
__device__ __forceinline__ bool point_in_tet(f3 v1, f3 v2, f3 v3, f3 v4, f3 p) {
	return same_side_tet(v1, v2, v3, v4, p) && same_side_tet(v2, v3, v4, v1, p) && same_side_tet(v3, v4, v1, v2, p) &&
	       same_side_tet(v4, v1, v2, v3, p);
}
__device__ __forceinline__ void bary_tet(f3 a, f3 b, f3 c, f3 d, f3 p, float out[4]) {
	f3 vap = p - a, vbp = p - b, vab = b - a, vac = c - a, vad = d - a, vbc = c - b, vbd = d - b;
	float va6 = scalar_tp(vbp, vbd, vbc);
	float vb6 = scalar_tp(vap, vac, vad);
	float vc6 = scalar_tp(vap, vad, vab);
	float vd6 = scalar_tp(vap, vab, vac);
	float v6 = (float)(1. / (double)scalar_tp(vab, vac, vad)); // the reference divides in double ("1. / float")
	out[0] = va6 * v6; out[1] = vb6 * v6; out[2] = vc6 * v6; out[3] = vd6 * v6;
}

// point_in_tet with the per-tet part of same_side_tet hoisted out of the sample loop, and the tet's own vertices stored next to
// it: tet_planes_kernel writes one 128-byte record per tet -- vertices v_0..v_3 (12 floats), normal_f = cross(v_{f+1} - v_f,
// v_{f+2} - v_f) for f = 0..3 (12 floats), the four bits signbit(dot(normal_f, v_{f+3} - v_f)) -- the very floats same_side_tet
// computes, so dot(normal_f, p - v_f) and the sign comparison are bit-identical to the direct evaluation.  One cache line per
// candidate instead of the tets[] -> vertices[] chain, and a quarter of the arithmetic.
__device__ __forceinline__ bool point_in_tet_rec(const float* __restrict__ recs, uint32_t t, f3 p) {
	typedef float f4n __attribute__((ext_vector_type(4))); // (a native vector: HIP's float4 is a class whose copy constructor wants a generic reference)
	const NRS_GLOBAL f4n* q = gp(reinterpret_cast<const f4n*>(recs)) + 8 * (size_t)t;
	const f4n v0 = q[0], v1 = q[1], v2 = q[2], n0 = q[3], n1 = q[4], n2 = q[5], sg = q[6];
	const float d0 = dot3(mk3(n0.x, n0.y, n0.z), p - mk3(v0.x, v0.y, v0.z));
	const float d1 = dot3(mk3(n0.w, n1.x, n1.y), p - mk3(v0.w, v1.x, v1.y));
	const float d2 = dot3(mk3(n1.z, n1.w, n2.x), p - mk3(v1.z, v1.w, v2.x));
	const float d3 = dot3(mk3(n2.y, n2.z, n2.w), p - mk3(v2.y, v2.z, v2.w));
	const uint32_t got = (__float_as_uint(d0) >> 31) | ((__float_as_uint(d1) >> 31) << 1) | ((__float_as_uint(d2) >> 31) << 2) | ((__float_as_uint(d3) >> 31) << 3);
	return got == __float_as_uint(sg.x);
}
// first tet of the list idx[j0 .. j1) that contains p (0xffffffff: none), t = idx[j0] already in hand; the next candidate's id is fetched while the current one is tested
__device__ __forceinline__ uint32_t scan_entries_for_tet(const DeviceEdit& e, const NRS_GLOBAL uint32_t* lut_idx, uint32_t j0, uint32_t j1, uint32_t t, f3 p, uint32_t* n_tested) {
	uint32_t found = 0xffffffffu;
	#pragma unroll 1
	for (uint32_t j = j0; j < j1; ++j) {
		const uint32_t t_next = lut_idx[min(j + 1, j1 - 1)];
		if (n_tested) ++*n_tested; // (profiling instantiation only)
		if (point_in_tet_rec(e.planes, t, p)) { found = t; break; }
		t = t_next;
	}
	return found;
}
// first tet of the cell's list that contains p (0xffffffff: none)
__device__ __forceinline__ uint32_t scan_list_for_tet(const DeviceEdit& e, const uint32_t* __restrict__ off, const uint32_t* __restrict__ idx, uint32_t cell, f3 p, uint32_t* n_tested = nullptr) {
	const NRS_GLOBAL uint32_t* lut_off = gp(off);
	const NRS_GLOBAL uint32_t* lut_idx = gp(idx);
	const uint32_t j0 = lut_off[cell], j1 = lut_off[cell + 1];
	if (j0 >= j1) return 0xffffffffu;
	return scan_entries_for_tet(e, lut_idx, j0, j1, lut_idx[j0], p, n_tested);
}
__device__ __forceinline__ uint32_t scan_cell_for_tet(const DeviceEdit& e, uint32_t cell, f3 p, uint32_t* n_tested = nullptr) { return scan_list_for_tet(e, e.lut_off, e.lut_idx, cell, p, n_tested); }
// the same scan of a fine cell through its head word (DeviceEdit::fine_head): one 8-byte load brings the list's start, its length and its first tet -- the two offsets and
// fine_idx[j0] of the scan above, two dependent trips -- so the first candidate's record and the second candidate's id are requested together.  The same candidates in
// the same order: the same tet.
__device__ __forceinline__ uint32_t scan_fine_cell_for_tet(const DeviceEdit& e, uint32_t cell, f3 p, uint32_t* n_tested = nullptr) {
	typedef uint32_t u2n __attribute__((ext_vector_type(2))); // (a native vector, as in point_in_tet_rec: one 8-byte load)
	const u2n head = *reinterpret_cast<const NRS_GLOBAL u2n*>(gp(e.fine_head) + cell);
	const uint32_t n = head.y >> kFineHeadTetBits;
	return scan_entries_for_tet(e, gp(e.fine_idx), head.x, head.x + n, head.y & ((1u << kFineHeadTetBits) - 1u), p, n_tested); // (n == 0: no iteration, nothing is read)
}
// The tet of e's deformed mesh that contains position u (un-warped), as the reference's scan of u's LUT cell finds it (0xffffffff: none).  With a fine look-up table
// (DeviceEdit::fine_off) the candidates are the fine cell's -- the same first hit by construction (nrs_cage.hip: fine_lists_kernel), after fewer tests: on the bench's cage
// the scan of a wave drops from 7 dependent trips per round to 2-3.  The fine coordinates are the LUT cell's arithmetic with a finer multiplier (cn:117-141), so fine >> shift
// IS the LUT cell; a position outside the window stands in a LUT cell whose list is empty.
// SHORT = false: the window per lane and the list through its CSR offsets, as before the head words -- for the gated kernel of the cone-stepping scenes, whose frame
// measured 0.4 % slower with the shorter chain (profiles/warp_chain.md: garden_cage; waves of several cascades, a tenth of the samples in the box)
template <bool SHORT = true>
__device__ __forceinline__ uint32_t find_tet(const DeviceEdit& e, f3 u, const uint32_t* __restrict__ march_lds, uint32_t* n_tested = nullptr) {
	const int level = mip_from_pos(u);
	if (e.fine_off) {
		typedef int32_t i4n __attribute__((ext_vector_type(4)));
		// The cascade's window.  Where every lane of the wave stands in the same cascade (always so in a scene box of scale 1, mostly so in larger ones) the eight ints
		// come in through scalar loads -- no trip of the vector memory path in front of the scan; the operator's struct does not change while a kernel runs.  (A pointer
		// with an explicit address space, like the views table's: one that could be merged with a pointer into the kernel arguments has them copied to scratch.  Where
		// `e` is a by-value kernel argument (map_rays_kernel; the render kernel and the occupancy refresh read their operators from a table in device memory) both casts below hold only because the compiler
		// leaves the struct in the kernel-argument segment, which is global and constant memory, and makes no private copy of it: the per-lane cast relied on that
		// before this one did; tests/test_gpu_parity.py::test_map_rays_bit_exact and tests/test_gpu_warp_chain.py run that kernel.)
		i4n lo, ext;
		const int level_u = __builtin_amdgcn_readfirstlane(level);
		if (SHORT && __all(level == level_u)) {
			const NRS_CONSTANT i4n* win = (const NRS_CONSTANT i4n*)reinterpret_cast<const i4n*>(&e.fine_win[0][0]) + 2 * level_u;
			lo = win[0]; ext = win[1];
		} else {
			const NRS_GLOBAL i4n* win = gp(reinterpret_cast<const i4n*>(&e.fine_win[0][0])) + 2 * level;
			lo = win[0]; ext = win[1];
		}
		const float mip_scale = ldexpf(1.0f, -level);
		f3 q = u - mk3(0.5f, 0.5f, 0.5f);
		q = q * mip_scale;
		q = q + mk3(0.5f, 0.5f, 0.5f);
		if (ext.w != kFinePlain) { // (else: this cascade keeps the LUT's own lists -- below)
			const int fres_i = (int)(kGrid << ext.w);
			const float fres = (float)fres_i;
			const int hi = fres_i - 1;
			const int fx = clampi_((int)(q.x * fres), 0, hi) - lo.x, fy = clampi_((int)(q.y * fres), 0, hi) - lo.y, fz = clampi_((int)(q.z * fres), 0, hi) - lo.z;
			if ((uint32_t)fx >= (uint32_t)ext.x || (uint32_t)fy >= (uint32_t)ext.y || (uint32_t)fz >= (uint32_t)ext.z) return 0xffffffffu;
			const uint32_t cell = (uint32_t)lo.w + ((uint32_t)fz * (uint32_t)ext.y + (uint32_t)fy) * (uint32_t)ext.x + (uint32_t)fx;
			if (SHORT && e.fine_head) return scan_fine_cell_for_tet(e, cell, u, n_tested);
			return scan_list_for_tet(e, e.fine_off, e.fine_idx, cell, u, n_tested);
		}
	}
	const uint32_t cell = march_lds ? occupancy_bit_index(u, (uint32_t)level, march_lds) : (uint32_t)level * kGridVol + cascaded_grid_idx_at(u, (uint32_t)level);
	return scan_cell_for_tet(e, cell, u, n_tested);
}

// interpolate_tet (with_dir, honours copy) / interpolate_tet_pos (!with_dir, ignores copy).  pos/dir are the warped
// [0,1] values of the NerfCoordinate; returns true if the sample must be treated as empty space.
// Two phases on purpose: the LUT scan only decides WHICH tet contains the sample; the barycentric map-back reloads that
// tet's vertices afterwards (from its plane record).  Fusing them keeps ~48 more VGPRs live across the scan and costs the kernel a wave of occupancy.
// march_lds (optional): the kernel's LDS copy of the Morton spread table (stage_march_lds) -- the cell index then costs three LDS reads instead of 28 VALU
// instructions (the same index: occupancy_bit_index is cascaded_grid_idx_at through the table)
// scan_out (optional): what the tet search found (a tet number or 0xffffffff), kTetNotSearched when the sample is outside the deformed mesh's box -- the membrane
// correction of the same operator looks for the same tet at the same position (poisson_residual_find) and takes it from here.
// RECORD = false: the map-back through tets -> verts -> orig -> rot, four dependent trips, as before the map-back records -- for the instantiation that has no
// register to spare for the record's wider trip (the membrane kernel: 128 VGPRs and scratch already); the same values, the same arithmetic.
constexpr uint32_t kTetNotSearched = 0xfffffffeu;
template <bool RECORD = true, bool SHORT = true> // (SHORT: find_tet's)
__device__ __forceinline__ bool tet_warp(const DeviceEdit& e, bool with_dir, f3& wpos, f3& wdir, const uint32_t* __restrict__ march_lds = nullptr, uint32_t* scan_out = nullptr,
                                         uint32_t* n_tested = nullptr) {
	bool in_deformed = false;
	if (scan_out) *scan_out = kTetNotSearched;
	if (box_contains(e.warped_bbox, wpos)) {
		const f3 u = unwarp_position(wpos, e.aabb);
		if (n_tested) *n_tested |= 0x10000u; // (profiling: the sample stands inside the deformed mesh's box; low half = candidates tested)
		const uint32_t found = find_tet<SHORT>(e, u, march_lds, n_tested);
		if (n_tested && found != 0xffffffffu) *n_tested |= 0x20000u;
		if (scan_out) *scan_out = found;
		__builtin_amdgcn_sched_barrier(0);
		if (found != 0xffffffffu) {
			// Everything the map-back reads of the tet hangs on `found` alone: its deformed vertices are the first 12 floats of its plane record (tet_planes_kernel copies
			// them there: the floats ld3(e.verts, tets[found].*) returns, in the line the scan has just read), its canonical vertices and its rotation are its map-back
			// record (DeviceEdit::mapback).  Vertices of both kinds in one trip, the rotation in a second -- where tets[found] -> verts -> orig -> rot were four
			// dependent trips.  The arithmetic is what it was, value for value.
			if constexpr (!RECORD) {
				typedef uint32_t u4n __attribute__((ext_vector_type(4)));
				const u4n tv = gp(reinterpret_cast<const u4n*>(e.tets))[found];
				float bc[4];
				{
					const f3 a = ld3(e.verts, tv.x), b = ld3(e.verts, tv.y), c = ld3(e.verts, tv.z), d = ld3(e.verts, tv.w);
					bary_tet(a, b, c, d, u, bc);
				}
				__builtin_amdgcn_sched_barrier(0);
				f3 canon = bc[0] * ld3(e.orig, tv.x) + bc[1] * ld3(e.orig, tv.y);
				canon = canon + bc[2] * ld3(e.orig, tv.z);
				canon = canon + bc[3] * ld3(e.orig, tv.w);
				wpos = e.diag_pow2 ? mk3((canon.x - e.aabb.mn[0]) * e.inv_diag[0], (canon.y - e.aabb.mn[1]) * e.inv_diag[1], (canon.z - e.aabb.mn[2]) * e.inv_diag[2])
				                   : warp_position(canon, e.aabb);
				__builtin_amdgcn_sched_barrier(0);
				if (with_dir && e.rot) {
					const f3 ud = unwarp_direction(wdir);
					const f3 c0 = ld3(e.rot, 3u * found), c1 = ld3(e.rot, 3u * found + 1u), c2 = ld3(e.rot, 3u * found + 2u); // the three columns
					const float R[9] = {c0.x, c0.y, c0.z, c1.x, c1.y, c1.z, c2.x, c2.y, c2.z};
					const f3 rd = mat3_mul(R, ud);
					wdir = warp_direction(rd);
				}
			} else {
				typedef float f4n __attribute__((ext_vector_type(4)));
				const NRS_GLOBAL f4n* pq = gp(reinterpret_cast<const f4n*>(e.planes)) + 8 * (size_t)found;
				const NRS_GLOBAL f4n* mq = gp(reinterpret_cast<const f4n*>(e.mapback)) + 6 * (size_t)found;
				const bool rotate = with_dir && e.rot;
				const f4n v0 = pq[0], v1 = pq[1], v2 = pq[2];
				const f4n o0 = mq[0], o1 = mq[1], o2 = mq[2];
				float bc[4];
				bary_tet(mk3(v0.x, v0.y, v0.z), mk3(v0.w, v1.x, v1.y), mk3(v1.z, v1.w, v2.x), mk3(v2.y, v2.z, v2.w), u, bc);
				// (the rotation behind bary_tet, where the twelve vertex registers are free again: with all nine words requested at once the default instantiation needs
				// 129 VGPRs and loses its fourth wave per SIMD -- so a second trip, whose data arrives under the canonical sum)
				__builtin_amdgcn_sched_barrier(0);
				f4n r0 = {0.f, 0.f, 0.f, 0.f}, r1 = {0.f, 0.f, 0.f, 0.f};
				float r2 = 0.f;
				if (rotate) { r0 = mq[3]; r1 = mq[4]; r2 = reinterpret_cast<const NRS_GLOBAL float*>(mq)[20]; }
				f3 canon = bc[0] * mk3(o0.x, o0.y, o0.z) + bc[1] * mk3(o0.w, o1.x, o1.y);
				canon = canon + bc[2] * mk3(o1.z, o1.w, o2.x);
				canon = canon + bc[3] * mk3(o2.y, o2.z, o2.w);
				wpos = e.diag_pow2 ? mk3((canon.x - e.aabb.mn[0]) * e.inv_diag[0], (canon.y - e.aabb.mn[1]) * e.inv_diag[1], (canon.z - e.aabb.mn[2]) * e.inv_diag[2])
				                   : warp_position(canon, e.aabb);
				if (rotate) {
					const f3 ud = unwarp_direction(wdir);
					const float R[9] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2}; // the three columns
					const f3 rd = mat3_mul(R, ud);
					wdir = warp_direction(rd);
				}
			}
			in_deformed = true;
		}
	}
	bool empty = false;
	if (!(with_dir && e.copy)) {
		if (!in_deformed && box_contains(e.orig_warped_bbox, wpos)) {
			const f3 u = unwarp_position(wpos, e.aabb);
			const int level = mip_from_pos(u);
			const uint32_t pos_idx = cascaded_grid_idx_at(u, (uint32_t)level);
			empty = gp(e.orig_bitfield)[pos_idx / 8 + (kGridVol * (uint32_t)level) / 8] & (1 << (pos_idx % 8)); // get_bitfield_at
		}
	}
	return empty;
}

// AffineDuplication::map_rays / map_positions (affine_duplication.cu:69-118): samples inside the warped destination box
// are carried back into the selection box (inverse scale, inverse rotation about the destination centre, inverse
// translation; optionally the view direction too); samples inside the selection box are emptied if hide_original.
__device__ __forceinline__ bool affine_contains(const AffineBox& b, f3 p) {
	const f3 q = p - mk3(b.mn[0], b.mn[1], b.mn[2]);
	const float du = dot3(mk3(b.u[0], b.u[1], b.u[2]), q), dv = dot3(mk3(b.v[0], b.v[1], b.v[2]), q), dw = dot3(mk3(b.w[0], b.w[1], b.w[2]), q);
	return du >= 0.f && du < b.uu && dv >= 0.f && dv < b.vv && dw >= 0.f && dw < b.ww;
}
__device__ __forceinline__ f3 mul_rt(const float* R, f3 q) { // R^T q, R column-major: (R^T q)_i = sum_k R(k, i) q_k
	return {sum3(R[0] * q.x, R[1] * q.y, R[2] * q.z), sum3(R[3] * q.x, R[4] * q.y, R[5] * q.z), sum3(R[6] * q.x, R[7] * q.y, R[8] * q.z)};
}
__device__ __forceinline__ bool affine_warp(const DeviceEdit& e, bool with_dir, f3& wpos, f3& wdir) {
	if (affine_contains(e.a_dst, wpos)) {
		const f3 c = mk3(e.a_dst.center[0], e.a_dst.center[1], e.a_dst.center[2]);
		const f3 d = wpos - c;
		const f3 q = {d.x / e.a_scale[0], d.y / e.a_scale[1], d.z / e.a_scale[2]};
		f3 p = mul_rt(e.a_rot, q) + c;
		wpos = p - mk3(e.a_translation[0], e.a_translation[1], e.a_translation[2]);
		if (with_dir && e.a_correct_dir) wdir = warp_direction(mul_rt(e.a_rot, unwarp_direction(wdir)));
		return false;
	}
	return e.a_hide_original && affine_contains(e.a_sel, wpos);
}
// EditOperator::map_rays / map_positions dispatch
template <bool RECORD = true> // (tet_warp's)
__device__ __forceinline__ bool edit_warp(const DeviceEdit& e, bool with_dir, f3& wpos, f3& wdir) {
	if (e.kind == kEditAffine) return affine_warp(e, with_dir, wpos, wdir);
	return tet_warp<RECORD>(e, with_dir, wpos, wdir);
}

// Membrane ("Poisson") correction inputs of one sample: compute_residual_poisson_kernel's body (cage_deformation.cu:467-507)
// fused with the evaluate_sh9 (cn:218-245) that composite_kernel_nerf applies to its result (tn:800-805).  wpos0 is the
// sample position BEFORE map_rays (residuals live in deformed space), dir the un-warped view direction AFTER map_rays.
// The barycentric interpolation of the 27 SH9RGB coefficients and the dot product with the SH basis are evaluated in the
// reference's order, coefficient by coefficient, so no 27-float array is kept.  Outputs untouched when no tet contains it.
// Two steps (round 4), so that the renderer can run the un-deformed network pass between them with only three values live: _find decides which tet of the
// deformed mesh holds the sample and interpolates the two densities; _colour re-derives the barycentric weights of that tet (the same arithmetic: the same
// bits) and evaluates the SH9 colour.
// searched (optional): the result of tet_warp's search of THIS operator's mesh at THIS position (the first operator the sample met: its position was still wpos0), or
// kTetNotSearched -- the same function of the same arguments, so it is taken instead of searched for again.
__device__ __forceinline__ bool poisson_residual_find(const DeviceEdit& e, f3 wpos0, uint32_t& found_out, float& out_density, float& res_density,
                                                      const uint32_t* __restrict__ march_lds = nullptr, uint32_t searched = kTetNotSearched) {
	const f3 pos = unwarp_position(wpos0, e.aabb);
	if (!box_contains(e.bbox, pos)) return false;
	uint32_t found = searched;
	if (searched == kTetNotSearched) {
		found = find_tet(e, pos, march_lds);
	}
	if (found == 0xffffffffu) return false;
	typedef uint32_t u4n __attribute__((ext_vector_type(4)));
	const u4n tv = gp(reinterpret_cast<const u4n*>(e.tets))[found];
	float bc[4];
	{
		const f3 a = ld3(e.verts, tv.x), b = ld3(e.verts, tv.y), c = ld3(e.verts, tv.z), dd = ld3(e.verts, tv.w);
		bary_tet(a, b, c, dd, pos, bc);
	}
	const NRS_GLOBAL float* od = gp(e.out_density);
	const NRS_GLOBAL float* rd = gp(e.res_density);
	const float lo = ((bc[0] * od[tv.x] + bc[1] * od[tv.y]) + bc[2] * od[tv.z]) + bc[3] * od[tv.w];
	const float lr = ((bc[0] * rd[tv.x] + bc[1] * rd[tv.y]) + bc[2] * rd[tv.z]) + bc[3] * rd[tv.w];
	out_density = e.residual_amplitude * lo;
	res_density = e.residual_amplitude * lr;
	found_out = found;
	return true;
}
__device__ __forceinline__ void poisson_residual_colour(const DeviceEdit& e, uint32_t found, f3 wpos0, f3 dir, float rgb[3]) {
	const f3 pos = unwarp_position(wpos0, e.aabb);
	typedef uint32_t u4n __attribute__((ext_vector_type(4)));
	const u4n tv = gp(reinterpret_cast<const u4n*>(e.tets))[found];
	float bc[4];
	{
		const f3 a = ld3(e.verts, tv.x), b = ld3(e.verts, tv.y), c = ld3(e.verts, tv.z), dd = ld3(e.verts, tv.w);
		bary_tet(a, b, c, dd, pos, bc);
	}
	// The 4 x 27 coefficients are read through a buffer descriptor (wave-uniform base in scalar registers, one 32-bit offset per vertex, the coefficient in
	// the instruction's immediate) and in small groups: the registers of a wave, not the latency of a few more round trips, are what this instantiation is
	// short of (the kernel must fit the 128 VGPRs of the default launch shape).  Two terms of the dot product are in flight at once.
	// (Round 6 measured the other extreme: a colour's nine coefficients of a vertex as two 16-byte loads + one dword, the interpolation vertex by vertex over all nine --
	// 36 loads and 6 round trips per sample instead of 108 in 15 groups: 54 spilled registers instead of 21 and the frame 3 % SLOWER, 9.42 against 9.72 Gsamples/s on one
	// box; one vertex in flight at a time: 9.36.  profiles/r06/ab_membrane_sh_*.txt.)
	const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)e.shs, 0, 0x7fffffff, 0x00020000);
	const uint32_t o0 = tv.x * 108u, o1 = tv.y * 108u, o2 = tv.z * 108u, o3 = tv.w * 108u; // byte offset of a vertex's 27 floats
	#pragma unroll 1 // one colour at a time (the unrolled form holds all 108 coefficient loads in flight: 250 VGPRs)
	for (int c = 0; c < 3; ++c) {
		const int cb = c * 36;
		// SH basis (evaluate_sh9, cn:222-240), each coefficient formed where it is used from an opaque copy of the direction: nine basis values kept across
		// the colour loop are nine registers this instantiation does not have (the products are the reference's, term by term)
		const float dx = dir.x, dy = dir.y, dz = dir.z;
		auto pSH = [&](int k) -> float {
			switch (k) {
				case 0: return 0.2820947917738781f;
				case 1: return -0.48860251190292f * dy;                          // fTmpA * fS0
				case 2: return 0.4886025119029199f * dz;
				case 3: return -0.48860251190292f * dx;                          // fTmpA * fC0
				case 4: return 0.5462742152960395f * (dx * dy + dy * dx);         // fTmpC * fS1
				case 5: return (-1.092548430592079f * dz) * dy;                  // fTmpB * fS0
				case 6: return 0.9461746957575601f * (dz * dz) + -0.3153915652525201f;
				case 7: return (-1.092548430592079f * dz) * dx;                  // fTmpB * fC0
				default: return 0.5462742152960395f * (dx * dx - dy * dy);       // fTmpC * fC1
			}
		};
		// pSH.dot(sh.block<9, 1>(0, c)): Eigen's unrolled 9-term reduction, 4 | 5 -> (2|2) | (2|(1|2))
		auto L = [&](uint32_t ov, int k) { return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, (int)ov, cb + 4 * k, 0)); };
		auto term = [&](int k) { return pSH(k) * (((bc[0] * L(o0, k) + bc[1] * L(o1, k)) + bc[2] * L(o2, k)) + bc[3] * L(o3, k)); };
		const float q0 = term(0), q1 = term(1); const float a01 = q0 + q1;
		__builtin_amdgcn_sched_barrier(0);
		const float q2 = term(2), q3 = term(3); const float lo4 = a01 + (q2 + q3);
		__builtin_amdgcn_sched_barrier(0);
		const float q4 = term(4), q5 = term(5); const float a45 = q4 + q5;
		__builtin_amdgcn_sched_barrier(0);
		const float q7 = term(7), q8 = term(8); const float a78 = q7 + q8;
		__builtin_amdgcn_sched_barrier(0);
		const float q6 = term(6);
		rgb[c] = lo4 + (a45 + (q6 + a78));
	}
}
// (the two steps in one call, for callers without anything in between)
__device__ __forceinline__ void poisson_residual_rgb(const DeviceEdit& e, f3 wpos0, f3 dir, float rgb[3], float& out_density, float& res_density) {
	uint32_t found;
	if (poisson_residual_find(e, wpos0, found, out_density, res_density)) poisson_residual_colour(e, found, wpos0, dir, rgb);
}

// compute_poisson_residual_density_kernel, cage_deformation.cu:341-384.  wpos is the position AFTER map_positions; the
// look-up nevertheless uses the deformed mesh's LUT, as the reference does.
__device__ __forceinline__ bool poisson_residual_density(const DeviceEdit& e, f3 wpos, float& residual) {
	const f3 pos = unwarp_position(wpos, e.aabb);
	if (!box_contains(e.bbox, pos)) return false;
	const uint32_t t = find_tet(e, pos, nullptr);
	if (t == 0xffffffffu) return false;
	const uint4 tv = reinterpret_cast<const uint4*>(e.tets)[t];
	const f3 a = ld3(e.verts, tv.x), b = ld3(e.verts, tv.y), c = ld3(e.verts, tv.z), d = ld3(e.verts, tv.w);
	float bc[4];
	bary_tet(a, b, c, d, pos, bc);
	residual = ((bc[0] * e.res_density[tv.x] + bc[1] * e.res_density[tv.y]) + bc[2] * e.res_density[tv.z]) + bc[3] * e.res_density[tv.w];
	return true;
}

} // namespace nrs
