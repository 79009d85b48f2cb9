// nrs_mesh.hip -- marching cubes on a density lattice and the per-vertex passes behind it (gfx950).
//
//   mc_count_kernel      crossings and triangles per lattice point, numbered inside a block of kMcBlock points with wave ballots (no atomics).
//   tile_scan_kernel     (nrs_scan.hip) exclusive scan over the blocks' sums: one workgroup.
//   mc_emit_kernel       gen_vertices + gen_faces (marching_cubes.cu:217, :313) in the numbering the two passes above fixed: ascending (point, axis) / ascending cell, table order.
//   mc_1ring_kernel      accumulate_1ring (:267) as a gather per vertex over the cells round its lattice edge: the sequential sum, no float atomics.
//   mesh_color_*         generate_nerf_network_inputs_from_positions (tn:608) and extract_srgb_with_activation (tn:338) either side of the network operator.
//
// All four lattice passes are 1-D launches over the linear point index i = x + y * rx + z * rx * ry: loads are coalesced along x and the block order is the point order.
// They are bound by the lattice read (the eight corners of a cell come from three x-rows that neighbouring lanes and the L2 share); the case table sits in LDS.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include "../../include/nrs.h"
#include "nrs_internal.h"
#include "nrs_launch.h"
#include "nrs_mesh.h"
#include "nrs_vec.cuh"
#include "nrs_grid_math.cuh"
#include "nrs_shade.cuh"
#include "nrs_scan.cuh"

namespace nrs {

// lanes below this one whose bit is set in a wave ballot
__device__ __forceinline__ uint32_t lanes_below(unsigned long long ballot) {
	return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

struct McPoint { uint32_t x, y, z; };
__device__ __forceinline__ McPoint mc_point(const McGrid& g, uint32_t i) {
	const uint32_t res2 = g.res[0] * g.res[1];
	const uint32_t z = i / res2, r = i - z * res2, y = r / g.res[0];
	return {r - y * g.res[0], y, z};
}
__device__ __forceinline__ bool mc_has_cell(const McGrid& g, const McPoint& p) { return p.x + 1 < g.res[0] && p.y + 1 < g.res[1] && p.z + 1 < g.res[2]; }
// gen_faces' mask of the cell whose lowest corner is point i (which has a cell): bit c = density[corner c] > thresh, a NaN counts as not above
__device__ __forceinline__ uint32_t mc_mask(const McGrid& g, const float* __restrict__ d, uint32_t i) {
	const uint32_t r1 = g.res[0], r2 = g.res[0] * g.res[1];
	uint32_t m = 0;
	if (d[i] > g.thresh) m |= 1u;
	if (d[i + 1] > g.thresh) m |= 2u;
	if (d[i + 1 + r1] > g.thresh) m |= 4u;
	if (d[i + r1] > g.thresh) m |= 8u;
	if (d[i + r2] > g.thresh) m |= 16u;
	if (d[i + r2 + 1] > g.thresh) m |= 32u;
	if (d[i + r2 + 1 + r1] > g.thresh) m |= 64u;
	if (d[i + r2 + r1] > g.thresh) m |= 128u;
	return m;
}

static_assert(kMcBlock == 256, "a thread stages one byte of the 256 triangle counts");
__global__ __launch_bounds__(kMcBlock) void mc_count_kernel(const McGrid g, const float* __restrict__ d, const uint8_t* __restrict__ n_tris_of, uint32_t* __restrict__ code,
                                                             uint32_t* __restrict__ block_sums) {
	__shared__ uint8_t s_n_tris[256];
	s_n_tris[threadIdx.x] = n_tris_of[threadIdx.x];
	__syncthreads();
	const uint32_t i = blockIdx.x * kMcBlock + threadIdx.x;
	bool fx = false, fy = false, fz = false;
	uint32_t nt = 0;
	if (i < g.n) {
		const McPoint p = mc_point(g, i);
		const bool inside = d[i] > g.thresh;
		if (p.x + 1 < g.res[0]) fx = inside != (d[i + 1] > g.thresh);
		if (p.y + 1 < g.res[1]) fy = inside != (d[i + g.res[0]] > g.thresh);
		if (p.z + 1 < g.res[2]) fz = inside != (d[i + g.res[0] * g.res[1]] > g.thresh);
		if (mc_has_cell(g, p)) nt = s_n_tris[mc_mask(g, d, i)];
	}
	const unsigned long long bx = __ballot(fx), by = __ballot(fy), bz = __ballot(fz);
	const unsigned long long t0 = __ballot(nt & 1u), t1 = __ballot(nt & 2u), t2 = __ballot(nt & 4u), t3 = __ballot(nt & 8u);
	const uint32_t in_wave[2] = {(uint32_t)(__popcll(bx) + __popcll(by) + __popcll(bz)), (uint32_t)(__popcll(t0) + 2 * __popcll(t1) + 4 * __popcll(t2) + 8 * __popcll(t3))};
	uint32_t before[2], total[2]; // vertices, triangles
	block_combine_waves<kMcBlock, 2>(in_wave, before, total);
	const uint32_t v_before = before[0] + lanes_below(bx) + lanes_below(by) + lanes_below(bz);
	const uint32_t t_before = before[1] + lanes_below(t0) + 2u * lanes_below(t1) + 4u * lanes_below(t2) + 8u * lanes_below(t3);
	// v_before <= 3 * 255 (10 bits), t_before <= 10 * 255 (12 bits)
	if (i < g.n) code[i] = v_before | ((uint32_t)fx << 10) | ((uint32_t)fy << 11) | ((uint32_t)fz << 12) | (t_before << 16);
	if (threadIdx.x == 0) { block_sums[2 * blockIdx.x] = total[0]; block_sums[2 * blockIdx.x + 1] = total[1]; }
}

// number of the vertex on the lattice edge that leaves point j along `axis` (the caller knows it is crossed)
__device__ __forceinline__ uint32_t mc_vertex_at(const uint32_t* __restrict__ code, const uint32_t* __restrict__ block_offs, uint32_t j, uint32_t axis) {
	const uint32_t c = code[j];
	return block_offs[2 * (j / kMcBlock)] + (c & 1023u) + (uint32_t)__popc((c >> 10) & ((1u << axis) - 1u));
}
__device__ __forceinline__ uint32_t mc_first_triangle(const uint32_t* __restrict__ code, const uint32_t* __restrict__ block_offs, uint32_t j) {
	return block_offs[2 * (j / kMcBlock) + 1] + ((code[j] >> 16) & 4095u);
}
// the lattice edge behind cube edge e of the cell at point i: its point and axis (gen_faces' local_edges, :625-638)
__device__ __forceinline__ uint32_t mc_edge_point(const McGrid& g, uint32_t i, uint32_t e) {
	const uint32_t r1 = g.res[0], r2 = g.res[0] * g.res[1];
	// a nibble per edge, e = 0 lowest: bit 0 = +1 in x, bit 1 = +1 in y, bit 2 = +1 in z (0 1 2 0 | 4 5 6 4 | 0 1 3 2)
	const uint32_t sel = (uint32_t)(0x231046540210ull >> (4u * e)) & 7u;
	return i + (sel & 1u) + ((sel & 2u) ? r1 : 0u) + ((sel & 4u) ? r2 : 0u);
}
__device__ __forceinline__ uint32_t mc_edge_axis(uint32_t e) { return e >= 8u ? 2u : (e & 1u); }

__global__ __launch_bounds__(kMcBlock) void mc_emit_kernel(const McGrid g, const float* __restrict__ d, const int8_t* __restrict__ table, uint32_t row_len,
                                                            const uint32_t* __restrict__ code, const uint32_t* __restrict__ block_offs, float* __restrict__ verts,
                                                            uint32_t* __restrict__ vert_src, uint32_t* __restrict__ indices) {
	__shared__ int8_t s_table[256 * kMcRowCap];
	for (uint32_t k = threadIdx.x; k < 256u * row_len; k += kMcBlock) s_table[k] = table[k];
	__syncthreads();
	const uint32_t i = blockIdx.x * kMcBlock + threadIdx.x;
	if (i >= g.n) return;
	const uint32_t c = code[i];
	const uint32_t flags = (c >> 10) & 7u;
	const McPoint p = mc_point(g, i);
	if (flags) { // gen_vertices, :227-263
		uint32_t v = block_offs[2 * blockIdx.x] + (c & 1023u);
		const float f0 = d[i];
		const uint32_t stride[3] = {1u, g.res[0], g.res[0] * g.res[1]};
		#pragma unroll
		for (uint32_t a = 0; a < 3; ++a) {
			if (!(flags & (1u << a))) continue;
			const float f1 = d[i + stride[a]];
			const float dt = (g.thresh - f0) / (f1 - f0);
			float q[3] = {(float)p.x, (float)p.y, (float)p.z};
			q[a] = q[a] + dt;
			verts[3 * (size_t)v + 0] = q[0] * g.scale[0] + g.offset[0];
			verts[3 * (size_t)v + 1] = q[1] * g.scale[1] + g.offset[1];
			verts[3 * (size_t)v + 2] = q[2] * g.scale[2] + g.offset[2];
			vert_src[v] = i * 4u + a;
			++v;
		}
	}
	if (!mc_has_cell(g, p)) return;
	const uint32_t mask = mc_mask(g, d, i);
	if (mask == 0u || mask == 255u) return;
	const int8_t* row = s_table + mask * row_len; // gen_faces, :640-653
	size_t out = 3 * (size_t)mc_first_triangle(code, block_offs, i);
	for (uint32_t k = 0; k + 1u < row_len && row[k] >= 0; ++k) {
		const uint32_t e = (uint32_t)row[k];
		indices[out++] = mc_vertex_at(code, block_offs, mc_edge_point(g, i, e), mc_edge_axis(e));
	}
}

// The cells round the lattice edge (point, axis), lowest cell first.  b and c are the two other axes, b the one with the smaller stride; the cell at
// (point - db * b - dc * c) sees the edge as its cube edge kEdgeSeen[axis][db + 2 * dc].
__constant__ uint8_t kEdgeSeen[3][4] = {{0, 2, 4, 6}, {3, 1, 7, 5}, {8, 9, 11, 10}};

__global__ __launch_bounds__(256) void mc_1ring_kernel(const McGrid g, const float* __restrict__ d, const int8_t* __restrict__ table, uint32_t row_len,
                                                        const uint32_t* __restrict__ code, const uint32_t* __restrict__ block_offs, uint32_t n_verts,
                                                        const uint32_t* __restrict__ vert_src, const float* __restrict__ verts, const uint32_t* __restrict__ indices,
                                                        float4* __restrict__ smoothed, float* __restrict__ normals) {
	__shared__ int8_t s_table[256 * kMcRowCap];
	for (uint32_t k = threadIdx.x; k < 256u * row_len; k += 256u) s_table[k] = table[k];
	__syncthreads();
	const uint32_t v = blockIdx.x * 256u + threadIdx.x;
	if (v >= n_verts) return;
	const uint32_t src = vert_src[v];
	const uint32_t i = src >> 2, axis = src & 3u;
	const McPoint p = mc_point(g, i);
	const uint32_t pos[3] = {p.x, p.y, p.z};
	const uint32_t stride[3] = {1u, g.res[0], g.res[0] * g.res[1]};
	const uint32_t b = axis == 0u ? 1u : 0u, c = axis == 2u ? 1u : 2u;
	float sx = 0.f, sy = 0.f, sz = 0.f, sw = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
	for (uint32_t q = 0; q < 4; ++q) { // ascending cell index: (db, dc) = (1, 1), (0, 1), (1, 0), (0, 0)
		const uint32_t db = (q & 1u) ^ 1u, dc = (q >> 1) ^ 1u;
		if (pos[b] < db || pos[c] < dc) continue;                                   // no cell on that side: the lattice's low boundary ...
		if (pos[b] - db + 1u >= g.res[b] || pos[c] - dc + 1u >= g.res[c]) continue; // ... or its high one (pos[axis] + 1 < res[axis]: the edge exists)
		const uint32_t cell = i - db * stride[b] - dc * stride[c];
		const uint32_t mask = mc_mask(g, d, cell);
		const int8_t* row = s_table + mask * row_len;
		const int me = (int)kEdgeSeen[axis][db + 2u * dc];
		size_t tri = 3 * (size_t)mc_first_triangle(code, block_offs, cell);
		for (uint32_t k = 0; k + 3u < row_len && row[k] >= 0; k += 3u, tri += 3) {
			const int e0 = row[k], e1 = row[k + 1], e2 = row[k + 2];
			if (e0 != me && e1 != me && e2 != me) continue;
			const uint32_t ia = indices[tri], ib = indices[tri + 1], ic = indices[tri + 2]; // accumulate_1ring, :270-301
			const float ax = verts[3 * (size_t)ia], ay = verts[3 * (size_t)ia + 1], az = verts[3 * (size_t)ia + 2];
			const float bx = verts[3 * (size_t)ib], by = verts[3 * (size_t)ib + 1], bz = verts[3 * (size_t)ib + 2];
			const float cx = verts[3 * (size_t)ic], cy = verts[3 * (size_t)ic + 1], cz = verts[3 * (size_t)ic + 2];
			if (e0 == me) { sx += bx + cx; sy += by + cy; sz += bz + cz; }
			else if (e1 == me) { sx += ax + cx; sy += ay + cy; sz += az + cz; }
			else { sx += bx + ax; sy += by + ay; sz += bz + az; }
			sw += 2.f;
			const float ux = bx - ax, uy = by - ay, uz = bz - az, wx = ax - cx, wy = ay - cy, wz = az - cz; // (pb - pa) x (pa - pc)
			nx += uy * wz - uz * wy;
			ny += uz * wx - ux * wz;
			nz += ux * wy - uy * wx;
		}
	}
	smoothed[v] = make_float4(sx, sy, sz, sw);
	normals[3 * (size_t)v] = nx;
	normals[3 * (size_t)v + 1] = ny;
	normals[3 * (size_t)v + 2] = nz;
}

// ---- vertex colours: compute_mesh_vertex_colors (tn:4515-4536) either side of the network operator ------------------------------------------------------------
__global__ __launch_bounds__(256) void mesh_color_inputs_kernel(uint32_t n, const float* __restrict__ verts, const Box3 aabb, float* __restrict__ coords) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	const f3 pos = mk3(verts[3 * (size_t)i], verts[3 * (size_t)i + 1], verts[3 * (size_t)i + 2]);
	f3 dir = mk3(pos.x - 0.5f, pos.y - 0.5f, pos.z - 0.5f); // "outward pointing directions, for want of a better choice"
	const float sq = (dir.x * dir.x + dir.y * dir.y) + dir.z * dir.z; // Eigen's normalized(): left alone when the squared norm is not positive
	if (sq > 0.f) { const float len = sqrtf(sq); dir = mk3(dir.x / len, dir.y / len, dir.z / len); }
	const f3 wpos = warp_position(pos, aabb), wdir = warp_direction(dir);
	float* c = coords + 7 * (size_t)i;
	c[0] = wpos.x; c[1] = wpos.y; c[2] = wpos.z;
	c[3] = warp_dt(NRS_MIN_STEP);
	c[4] = wdir.x; c[5] = wdir.y; c[6] = wdir.z;
}
// the network's output is fp16, 16 channels per sample (NRS_INTERLEAVED); inference() hands the first four to the caller as float
__global__ __launch_bounds__(256) void mesh_colors_kernel(uint32_t n3, const __half* __restrict__ net, uint32_t rgb_activation, int linear_colors, float* __restrict__ colors) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n3) return;
	const uint32_t elem = i / 3u, dim = i - elem * 3u;
	float c = network_to_rgb(__half2float(net[16 * (size_t)elem + dim]), rgb_activation);
	if (linear_colors) c = c < 0.0031308f ? 12.92f * c : 1.055f * powf(c, 0.41666f) - 0.055f; // linear_to_srgb, common_device.cuh:55-61
	colors[i] = c;
}

static uint32_t mc_blocks(uint32_t n) { return (n + kMcBlock - 1) / kMcBlock; }

int launch_mc_count(const McGrid& g, const float* d_density, const uint8_t* d_n_tris, uint32_t* d_code, uint32_t* d_block_sums, void* stream) {
	hipLaunchKernelGGL(mc_count_kernel, dim3(mc_blocks(g.n)), dim3(kMcBlock), 0, (hipStream_t)stream, g, d_density, d_n_tris, d_code, d_block_sums);
	NRS_LAUNCH_CHECK("mc_count_kernel launch");
	return NRS_OK;
}
int launch_mc_emit(const McGrid& g, const float* d_density, const int8_t* d_table, uint32_t row_len, const uint32_t* d_code, const uint32_t* d_block_offs,
                   float* d_verts, uint32_t* d_vert_src, uint32_t* d_indices, void* stream) {
	if (row_len > kMcRowCap) { snprintf(g_launch_err, sizeof(g_launch_err), "mc_emit_kernel: case table row longer than %u", kMcRowCap); return NRS_ERR_STATE; }
	hipLaunchKernelGGL(mc_emit_kernel, dim3(mc_blocks(g.n)), dim3(kMcBlock), 0, (hipStream_t)stream, g, d_density, d_table, row_len, d_code, d_block_offs, d_verts, d_vert_src,
	                   d_indices);
	NRS_LAUNCH_CHECK("mc_emit_kernel launch");
	return NRS_OK;
}
int launch_mc_1ring(const McGrid& g, const float* d_density, const int8_t* d_table, uint32_t row_len, const uint32_t* d_code, const uint32_t* d_block_offs, uint32_t n_verts,
                    const uint32_t* d_vert_src, const float* d_verts, const uint32_t* d_indices, float* d_smoothed, float* d_normals, void* stream) {
	if (n_verts == 0) return NRS_OK;
	if (row_len > kMcRowCap) { snprintf(g_launch_err, sizeof(g_launch_err), "mc_1ring_kernel: case table row longer than %u", kMcRowCap); return NRS_ERR_STATE; }
	hipLaunchKernelGGL(mc_1ring_kernel, dim3((n_verts + 255) / 256), dim3(256), 0, (hipStream_t)stream, g, d_density, d_table, row_len, d_code, d_block_offs, n_verts, d_vert_src,
	                   d_verts, d_indices, reinterpret_cast<float4*>(d_smoothed), d_normals);
	NRS_LAUNCH_CHECK("mc_1ring_kernel launch");
	return NRS_OK;
}
int launch_mesh_color_inputs(uint32_t n, const float* d_verts, const Box3& aabb, float* d_coords7, void* stream) {
	if (n == 0) return NRS_OK;
	hipLaunchKernelGGL(mesh_color_inputs_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, d_verts, aabb, d_coords7);
	NRS_LAUNCH_CHECK("mesh_color_inputs_kernel launch");
	return NRS_OK;
}
int launch_mesh_colors(uint32_t n, const void* d_net_fp16, uint32_t rgb_activation, int linear_colors, float* d_colors, void* stream) {
	if (n == 0) return NRS_OK;
	hipLaunchKernelGGL(mesh_colors_kernel, dim3((3 * n + 255) / 256), dim3(256), 0, (hipStream_t)stream, 3 * n, reinterpret_cast<const __half*>(d_net_fp16), rgb_activation,
	                   linear_colors, d_colors);
	NRS_LAUNCH_CHECK("mesh_colors_kernel launch");
	return NRS_OK;
}

} // namespace nrs
