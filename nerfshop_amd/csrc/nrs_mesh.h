// nrs_mesh.h -- the launchers of nrs_mesh.hip and the lattice they walk.
#pragma once
#include <stdint.h>
#include "nrs_internal.h"

namespace nrs {

// marching cubes (nrs_mesh.hip).  The lattice is walked by its linear point index i = x + y * rx + z * rx * ry in blocks of kMcBlock points; a point owns the (up to three)
// vertices on its +x / +y / +z lattice edges and the triangles of the cell it is the lowest corner of.
constexpr uint32_t kMcBlock = 256;
constexpr uint32_t kMcRowCap = 32;   // a row of the case table: at most 10 triangles (12 crossed edges, one loop of k edges gives k - 2) and the terminator
struct McGrid {
	uint32_t res[3];
	uint32_t n;                      // res[0] * res[1] * res[2]
	float scale[3], offset[3];       // vertex = lattice position * scale + offset (product and sum separate)
	float thresh;
};
// per point: d_code = vertices before it in its block | crossing flags (x, y, z) << 10 | triangles before it in its block << 16; d_block_sums [2 * n_blocks] = vertices, triangles of a block
int launch_mc_count(const McGrid& g, const float* d_density, const uint8_t* d_n_tris /* [256] */, uint32_t* d_code, uint32_t* d_block_sums, void* stream);
// then launch_tile_scan(n_blocks, 2, d_block_sums, d_totals, ...): d_totals[2] = vertices, triangles of the lattice
// vertices (d_verts [n_verts x 3], d_vert_src [n_verts] = point * 4 + axis) and triangles (d_indices [n_tris x 3]) in ascending point order
int launch_mc_emit(const McGrid& g, const float* d_density, const int8_t* d_table, uint32_t row_len, const uint32_t* d_code, const uint32_t* d_block_offs,
                   float* d_verts, uint32_t* d_vert_src, uint32_t* d_indices, void* stream);
// accumulate_1ring as a gather: a vertex sums over the triangles of the (up to four) cells round its lattice edge, in ascending triangle order
int launch_mc_1ring(const McGrid& g, const float* d_density, const int8_t* d_table, uint32_t row_len, const uint32_t* d_code, const uint32_t* d_block_offs, uint32_t n_verts,
                    const uint32_t* d_vert_src, const float* d_verts, const uint32_t* d_indices, float* d_smoothed, float* d_normals, void* stream);
// generate_nerf_network_inputs_from_positions (tn:608): [n x 7] network inputs of n vertices; extract_srgb_with_activation (tn:338) on interleaved fp16 network outputs
int launch_mesh_color_inputs(uint32_t n, const float* d_verts, const Box3& aabb, float* d_coords7, void* stream);
int launch_mesh_colors(uint32_t n, const void* d_net_fp16, uint32_t rgb_activation, int linear_colors, float* d_colors, void* stream);

} // namespace nrs
