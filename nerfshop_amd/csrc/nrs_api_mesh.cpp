// nrs_api_mesh.cpp -- mesh extraction: the marching-cubes case table (generated here, from a rule), the resolution helper, the mesh handle, the file writers.
#include "nrs_handles.h"
#include "nrs_network.h"
#include "nrs_mesh.h"
#include "nrs_scan.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>

using namespace nrs;

struct nrs_mesh {
	int device = 0;
	uint32_t n_verts = 0, n_padded = 0, n_tris = 0;
	bool has_colors = false;
	DeviceBuffer<float> d_verts;       // [n_padded x 3], padding rows zero
	DeviceBuffer<float> d_normals;     // [n_padded x 3] area-weighted sums, not normalised
	DeviceBuffer<float> d_colors;      // [n_padded x 3] (nrs_mesh_extract only)
	DeviceBuffer<float> d_smoothed;    // [n_padded x 4] homogeneous 1-ring sums
	DeviceBuffer<uint32_t> d_indices;  // [n_tris x 3]
};

namespace {

// ---- the case table ------------------------------------------------------------------------------------------------------------------------------------------
// The cube in the reference's numbering: corners 0..3 round the z = 0 face, 4..7 above them; edges 0..3 / 4..7 round those faces, 8..11 in +z from corners 0..3.
constexpr int kEdgeEnds[12][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 0}, {4, 5}, {5, 6}, {6, 7}, {7, 4}, {0, 4}, {1, 5}, {2, 6}, {3, 7}};
// the six faces, corners counter-clockwise as seen from outside the cube: z = 0, z = 1, y = 0, x = 1, y = 1, x = 0
constexpr int kFaceCorners[6][4] = {{0, 3, 2, 1}, {4, 5, 6, 7}, {0, 1, 5, 4}, {1, 2, 6, 5}, {2, 3, 7, 6}, {3, 0, 4, 7}};

int edge_between(int a, int b) {
	for (int e = 0; e < 12; ++e)
		if ((kEdgeEnds[e][0] == a && kEdgeEnds[e][1] == b) || (kEdgeEnds[e][0] == b && kEdgeEnds[e][1] == a)) return e;
	return -1;
}
bool edges_share_face(int e0, int e1) {
	for (const auto& f : kFaceCorners) {
		int hits = 0;
		for (int k = 0; k < 4; ++k)
			for (int e : {e0, e1})
				for (int end = 0; end < 2; ++end) hits += kEdgeEnds[e][end] == f[k];
		if (hits == 4) return true; // all four ends (three corners when the edges touch, each counted once per edge) lie on the face
	}
	return false;
}

struct McTable {
	int8_t rows[256][kMcRowCap];
	uint8_t n_tris[256];
	uint32_t row_len; // the longest row and its terminator
};

// The rule.  On every face, walking its corners counter-clockwise as seen from outside, each maximal run of set corners is cut off by one
// segment, directed from the edge where the walk leaves the run to the edge where it entered it: two set corners on a diagonal are two runs, each cut off on its
// own, and the choice depends on that face's corner states alone.  Every crossed edge is left by one segment and reached by one, so the segments close into
// loops.  Loops are listed in order of their lowest edge; a loop is walked from that edge and fanned from the first edge on the walk whose fan puts no diagonal
// inside a cube face (the lowest edge itself for all but twenty loops).  With this direction (pb - pa) x (pa - pc) of a triangle (a, b, c) points to the unset side.
McTable generate_table() {
	McTable t{};
	t.row_len = 0;
	for (int mask = 0; mask < 256; ++mask) {
		int next[12];
		for (int& n : next) n = -1;
		for (const auto& f : kFaceCorners) {
			bool set[4];
			for (int k = 0; k < 4; ++k) set[k] = (mask >> f[k]) & 1;
			for (int k = 0; k < 4; ++k) {
				if (!(set[k] && !set[(k + 1) & 3])) continue; // the walk leaves a run behind corner k
				int j = k;
				while (set[(j + 3) & 3]) j = (j + 3) & 3;     // back to the run's first corner (not all four are set: corner k + 1 is not)
				next[edge_between(f[k], f[(k + 1) & 3])] = edge_between(f[(j + 3) & 3], f[j]);
			}
		}
		int8_t* row = t.rows[mask];
		uint32_t len = 0;
		bool seen[12] = {};
		for (int start = 0; start < 12; ++start) {
			if (next[start] < 0 || seen[start]) continue;
			int loop[12], k = 0;
			for (int e = start; !seen[e]; e = next[e]) { seen[e] = true; loop[k++] = e; }
			int apex = 0;
			for (; apex < k; ++apex) {
				bool flat = false;
				for (int i = 2; i < k - 1; ++i) flat |= edges_share_face(loop[apex], loop[(apex + i) % k]);
				if (!flat) break;
			}
			if (apex == k) apex = 0; // (does not happen: tests/test_marching_cubes_host.py checks every row)
			for (int i = 1; i < k - 1; ++i) {
				row[len++] = (int8_t)loop[apex];
				row[len++] = (int8_t)loop[(apex + i) % k];
				row[len++] = (int8_t)loop[(apex + i + 1) % k];
			}
		}
		t.n_tris[mask] = (uint8_t)(len / 3);
		for (uint32_t i = len; i < kMcRowCap; ++i) row[i] = -1;
		t.row_len = std::max(t.row_len, len + 1);
	}
	return t;
}
const McTable& mc_table() {
	static const McTable t = generate_table(); // at first use
	return t;
}

bool finite3(const float* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }
uint32_t next_multiple_16(uint32_t v) { return (v + 15u) / 16u * 16u; }

// what nrs_mesh_from_density and nrs_mesh_extract refuse in their lattice and box, before a device is touched
int check_lattice(const uint32_t res3d[3], const float aabb_min[3], const float aabb_max[3], float thresh, const char* fn) {
	const char* what = nullptr;
	if (res3d[0] < 2u || res3d[1] < 2u || res3d[2] < 2u) what = "res3d has an axis below 2";
	else if ((uint64_t)res3d[0] * res3d[1] >= (1ull << 31) || (uint64_t)res3d[0] * res3d[1] * res3d[2] > ((1ull << 31) - 1) / 3) what = "res3d: 3 * rx * ry * rz reaches 2^31";
	else if (!std::isfinite(thresh)) what = "thresh is not finite";
	else if (!finite3(aabb_min)) what = "aabb_min is not finite";
	else if (!finite3(aabb_max)) what = "aabb_max is not finite";
	else if (!(aabb_max[0] > aabb_min[0] && aabb_max[1] > aabb_min[1] && aabb_max[2] > aabb_min[2])) what = "aabb_max is not above aabb_min on every axis";
	if (!what) return NRS_OK;
	return fail(NRS_ERR_INVALID_ARG, std::string(fn) + ": " + what);
}

// marching_cubes_gpu (marching_cubes.cu:730-758) + compute_mesh_1ring (:656-662) on a lattice that is already on the device
int build_mesh(int device, void* stream, const uint32_t res3d[3], const float aabb_min[3], const float aabb_max[3], float thresh, const float* d_density,
               std::unique_ptr<nrs_mesh>& out, const char* fn) {
	const McTable& table = mc_table();
	McGrid g{};
	for (int k = 0; k < 3; ++k) {
		g.res[k] = res3d[k];
		g.scale[k] = (aabb_max[k] - aabb_min[k]) / (float)res3d[k]; // (aabb.max - aabb.min).cwiseQuotient(res_3d.cast<float>()), :222
		g.offset[k] = aabb_min[k];
	}
	g.n = res3d[0] * res3d[1] * res3d[2];
	g.thresh = thresh;
	const uint32_t n_blocks = (g.n + kMcBlock - 1) / kMcBlock;
	hipStream_t s = (hipStream_t)stream;

	DeviceBuffer<int8_t> d_table;          // [256 x row_len] rows | [256] triangle counts
	DeviceBuffer<uint32_t> d_code, d_block_sums, d_totals, d_vert_src;
	const size_t table_bytes = 256 * (size_t)table.row_len;
	hipError_t he = d_table.alloc(table_bytes + 256);
	if (he == hipSuccess) he = d_code.alloc(g.n);
	if (he == hipSuccess) he = d_block_sums.alloc(2 * (size_t)n_blocks);
	if (he == hipSuccess) he = d_totals.alloc(2);
	if (he != hipSuccess) return fail_hip(he, (std::string(fn) + ": device allocation (per-point codes)").c_str());
	std::vector<int8_t> packed(table_bytes + 256);
	for (int m = 0; m < 256; ++m) {
		memcpy(packed.data() + (size_t)m * table.row_len, table.rows[m], table.row_len);
		packed[table_bytes + m] = (int8_t)table.n_tris[m];
	}
	HIP_TRY(hipMemcpyAsync(d_table.get(), packed.data(), packed.size(), hipMemcpyHostToDevice, s));
	NRS_LAUNCH(launch_mc_count(g, d_density, reinterpret_cast<const uint8_t*>(d_table.get() + table_bytes), d_code.get(), d_block_sums.get(), s));
	NRS_LAUNCH(launch_tile_scan(n_blocks, 2, d_block_sums.get(), d_totals.get(), nullptr, s));
	uint32_t totals[2] = {0, 0};
	HIP_TRY(hipMemcpyAsync(totals, d_totals.get(), sizeof(totals), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s)); // the one synchronisation: the counts size the arrays (the reference reads its counters back the same way, :747-748)

	auto mesh = std::make_unique<nrs_mesh>();
	mesh->device = device;
	mesh->n_verts = totals[0];
	mesh->n_padded = (totals[0] + 127u) & ~127u; // "round for later nn stuff", :751
	mesh->n_tris = totals[1];
	const size_t np = mesh->n_padded;
	he = mesh->d_verts.alloc(np * 3);
	if (he == hipSuccess) he = mesh->d_normals.alloc(np * 3);
	if (he == hipSuccess) he = mesh->d_smoothed.alloc(np * 4);
	if (he == hipSuccess) he = mesh->d_indices.alloc((size_t)mesh->n_tris * 3);
	if (he == hipSuccess) he = d_vert_src.alloc(mesh->n_verts);
	if (he != hipSuccess) return fail_hip(he, (std::string(fn) + ": device allocation (mesh)").c_str());
	if (np) {
		HIP_TRY(hipMemsetAsync(mesh->d_verts.get(), 0, np * 3 * sizeof(float), s));
		HIP_TRY(hipMemsetAsync(mesh->d_normals.get(), 0, np * 3 * sizeof(float), s));
		HIP_TRY(hipMemsetAsync(mesh->d_smoothed.get(), 0, np * 4 * sizeof(float), s));
	}
	if (mesh->n_verts) {
		NRS_LAUNCH(launch_mc_emit(g, d_density, d_table.get(), table.row_len, d_code.get(), d_block_sums.get(), mesh->d_verts.get(), d_vert_src.get(), mesh->d_indices.get(), s));
		NRS_LAUNCH(launch_mc_1ring(g, d_density, d_table.get(), table.row_len, d_code.get(), d_block_sums.get(), mesh->n_verts, d_vert_src.get(), mesh->d_verts.get(),
		                           mesh->d_indices.get(), mesh->d_smoothed.get(), mesh->d_normals.get(), s));
	}
	HIP_TRY(hipStreamSynchronize(s)); // the temporaries go when this returns
	out = std::move(mesh);
	return NRS_OK;
}

// filesystem::path(outputname).extension() == "ply": what follows the last dot of the file name
bool has_ply_extension(const char* path) {
	const char* name = strrchr(path, '/');
	name = name ? name + 1 : path;
	const char* dot = strrchr(name, '.');
	return dot && strcmp(dot + 1, "ply") == 0;
}
float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); } // tcnn::clamp
void normalized(const float* v, float out[3]) { // Eigen's normalized(): a vector without a positive squared norm is left alone
	const float sq = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
	const float len = sq > 0.f ? std::sqrt(sq) : 1.f;
	for (int k = 0; k < 3; ++k) out[k] = sq > 0.f ? v[k] / len : v[k];
}

} // namespace

int nrs::mesh_from_lattice(int device, void* stream, const uint32_t res3d[3], const float aabb_min[3], const float aabb_max[3], float thresh, const float* d_density,
                           nrs_mesh** mesh_out, const char* fn) {
	std::unique_ptr<nrs_mesh> mesh;
	NRS_TRY(build_mesh(device, stream, res3d, aabb_min, aabb_max, thresh, d_density, mesh, fn));
	*mesh_out = mesh.release();
	return NRS_OK;
}

extern "C" {

// get_marching_cubes_res, marching_cubes.cu:48-55
int nrs_marching_cubes_res(uint32_t res_1d, const float aabb_min[3], const float aabb_max[3], uint32_t res3d_out[3]) {
	if (!aabb_min) return fail(NRS_ERR_INVALID_ARG, "nrs_marching_cubes_res: aabb_min is NULL");
	if (!aabb_max) return fail(NRS_ERR_INVALID_ARG, "nrs_marching_cubes_res: aabb_max is NULL");
	if (!res3d_out) return fail(NRS_ERR_INVALID_ARG, "nrs_marching_cubes_res: res3d_out is NULL");
	if (!finite3(aabb_min) || !finite3(aabb_max)) return fail(NRS_ERR_INVALID_ARG, "nrs_marching_cubes_res: aabb_min / aabb_max is not finite");
	const float d[3] = {aabb_max[0] - aabb_min[0], aabb_max[1] - aabb_min[1], aabb_max[2] - aabb_min[2]};
	const float longest = std::max(d[0], std::max(d[1], d[2]));
	if (!(d[0] >= 0.f && d[1] >= 0.f && d[2] >= 0.f && longest > 0.f)) return fail(NRS_ERR_INVALID_ARG, "nrs_marching_cubes_res: aabb_max is below aabb_min, or the box is empty");
	const float scale = (float)res_1d / longest;
	for (int k = 0; k < 3; ++k) {
		const float v = d[k] * scale + 0.5f;
		if (!(v < 2147483648.f)) return fail(NRS_ERR_INVALID_ARG, "nrs_marching_cubes_res: res_1d is too large");
		res3d_out[k] = next_multiple_16((uint32_t)(int)v);
	}
	return NRS_OK;
}

int nrs_marching_cubes_table(int8_t* out, uint32_t* row_len) {
	if (!row_len) return fail(NRS_ERR_INVALID_ARG, "nrs_marching_cubes_table: row_len is NULL");
	const McTable& t = mc_table();
	*row_len = t.row_len;
	if (out)
		for (int m = 0; m < 256; ++m) memcpy(out + (size_t)m * t.row_len, t.rows[m], t.row_len);
	return NRS_OK;
}

// save_mesh (marching_cubes.cu:760-896) without the unwrap branch
int nrs_mesh_write(const char* path, uint32_t n_verts, const float* h_verts, const float* h_normals, const float* h_colors, uint32_t n_tris, const uint32_t* h_indices,
                   float scale, const float offset[3]) {
	if (!path) return fail(NRS_ERR_INVALID_ARG, "nrs_mesh_write: path is NULL");
	if (n_verts && !h_verts) return fail(NRS_ERR_INVALID_ARG, "nrs_mesh_write: h_verts is NULL");
	if (n_verts && !h_normals) return fail(NRS_ERR_INVALID_ARG, "nrs_mesh_write: h_normals is NULL");
	if (n_verts && !h_colors) return fail(NRS_ERR_INVALID_ARG, "nrs_mesh_write: h_colors is NULL");
	if (n_tris && !h_indices) return fail(NRS_ERR_INVALID_ARG, "nrs_mesh_write: h_indices is NULL");
	if (!offset) return fail(NRS_ERR_INVALID_ARG, "nrs_mesh_write: offset is NULL");
	FILE* f = fopen(path, "wb");
	if (!f) return fail(NRS_ERR_INVALID_ARG, std::string("nrs_mesh_write: failed to open ") + path + " for writing");
	if (has_ply_extension(path)) {
		fprintf(f,
		        "ply\n"
		        "format ascii 1.0\n"
		        "comment output from https://github.com/NVlabs/instant-ngp\n"
		        "element vertex %u\n"
		        "property float x\n"
		        "property float y\n"
		        "property float z\n"
		        "property float nx\n"
		        "property float ny\n"
		        "property float nz\n"
		        "property uchar red\n"
		        "property uchar green\n"
		        "property uchar blue\n"
		        "element face %u\n"
		        "property list uchar int vertex_index\n"
		        "end_header\n",
		        n_verts, n_tris);
		for (uint32_t i = 0; i < n_verts; ++i) {
			const float* v = h_verts + 3 * (size_t)i;
			const float* c = h_colors + 3 * (size_t)i;
			float n[3];
			normalized(h_normals + 3 * (size_t)i, n);
			const float p[3] = {(v[0] - offset[0]) / scale, (v[1] - offset[1]) / scale, (v[2] - offset[2]) / scale};
			const unsigned char c8[3] = {(unsigned char)clampf(c[0] * 255.f, 0.f, 255.f), (unsigned char)clampf(c[1] * 255.f, 0.f, 255.f), (unsigned char)clampf(c[2] * 255.f, 0.f, 255.f)};
			fprintf(f, "%0.5f %0.5f %0.5f %0.3f %0.3f %0.3f %d %d %d\n", p[0], p[1], p[2], n[0], n[1], n[2], c8[0], c8[1], c8[2]);
		}
		for (size_t i = 0; i < (size_t)n_tris * 3; i += 3) fprintf(f, "3 %d %d %d\n", h_indices[i + 2], h_indices[i + 1], h_indices[i + 0]);
	} else {
		for (uint32_t i = 0; i < n_verts; ++i) {
			const float* v = h_verts + 3 * (size_t)i;
			const float* c = h_colors + 3 * (size_t)i;
			const float p[3] = {(v[0] - offset[0]) / scale, (v[1] - offset[1]) / scale, (v[2] - offset[2]) / scale};
			fprintf(f, "v %0.5f %0.5f %0.5f %0.3f %0.3f %0.3f\n", p[0], p[1], p[2], clampf(c[0], 0.f, 1.f), clampf(c[1], 0.f, 1.f), clampf(c[2], 0.f, 1.f));
		}
		for (uint32_t i = 0; i < n_verts; ++i) {
			float n[3];
			normalized(h_normals + 3 * (size_t)i, n);
			fprintf(f, "vn %0.5f %0.5f %0.5f\n", n[0], n[1], n[2]);
		}
		for (size_t i = 0; i < (size_t)n_tris * 3; i += 3)
			fprintf(f, "f %u//%u %u//%u %u//%u\n", h_indices[i + 2] + 1, h_indices[i + 2] + 1, h_indices[i + 1] + 1, h_indices[i + 1] + 1, h_indices[i + 0] + 1, h_indices[i + 0] + 1);
	}
	const bool bad = ferror(f) != 0;
	if (fclose(f) != 0 || bad) return fail(NRS_ERR_INVALID_ARG, std::string("nrs_mesh_write: writing ") + path + " failed");
	return NRS_OK;
}

int nrs_mesh_from_density(nrs_ctx* ctx, void* stream, const uint32_t res3d[3], const float aabb_min[3], const float aabb_max[3], float thresh, const float* d_density,
                          nrs_mesh** out) {
	if (!ctx) return fail(NRS_ERR_INVALID_ARG, "nrs_mesh_from_density: ctx is NULL");
	if (!res3d) return fail(NRS_ERR_INVALID_ARG, "nrs_mesh_from_density: res3d is NULL");
	if (!aabb_min) return fail(NRS_ERR_INVALID_ARG, "nrs_mesh_from_density: aabb_min is NULL");
	if (!aabb_max) return fail(NRS_ERR_INVALID_ARG, "nrs_mesh_from_density: aabb_max is NULL");
	if (!d_density) return fail(NRS_ERR_INVALID_ARG, "nrs_mesh_from_density: d_density is NULL");
	if (!out) return fail(NRS_ERR_INVALID_ARG, "nrs_mesh_from_density: mesh_out is NULL");
	NRS_TRY(check_lattice(res3d, aabb_min, aabb_max, thresh, "nrs_mesh_from_density"));
	HIP_TRY(hipSetDevice(ctx->device));
	std::unique_ptr<nrs_mesh> mesh;
	NRS_TRY(build_mesh(ctx->device, stream, res3d, aabb_min, aabb_max, thresh, d_density, mesh, "nrs_mesh_from_density"));
	*out = mesh.release();
	return NRS_OK;
}

// generate_nerf_network_inputs_from_positions (testbed_nerf.cu:608-614) for the padded rows of a mesh
int nrs_mesh_color_inputs(nrs_model* model, void* stream, const nrs_mesh* mesh, float* d_coords_out) {
	if (!model) return fail(NRS_ERR_INVALID_ARG, "nrs_mesh_color_inputs: model is NULL");
	if (!mesh) return fail(NRS_ERR_INVALID_ARG, "nrs_mesh_color_inputs: mesh is NULL");
	if (!d_coords_out) return fail(NRS_ERR_INVALID_ARG, "nrs_mesh_color_inputs: d_coords_out is NULL");
	HIP_TRY(hipSetDevice(model->ctx->device));
	NRS_LAUNCH(launch_mesh_color_inputs(mesh->n_padded, mesh->d_verts.get(), model->dm.aabb, d_coords_out, stream));
	return NRS_OK;
}

// Testbed::marching_cubes (testbed_nerf.cu:4614-4649) without the optimiser state
int nrs_mesh_extract(nrs_model* model, void* stream, const uint32_t res3d[3], const float aabb_min[3], const float aabb_max[3], float thresh, int mask_with_density_grid,
                     int linear_colors, nrs_mesh** out) {
	if (!model) return fail(NRS_ERR_INVALID_ARG, "nrs_mesh_extract: model is NULL");
	if (!res3d) return fail(NRS_ERR_INVALID_ARG, "nrs_mesh_extract: res3d is NULL");
	if (!aabb_min) return fail(NRS_ERR_INVALID_ARG, "nrs_mesh_extract: aabb_min is NULL");
	if (!aabb_max) return fail(NRS_ERR_INVALID_ARG, "nrs_mesh_extract: aabb_max is NULL");
	if (!out) return fail(NRS_ERR_INVALID_ARG, "nrs_mesh_extract: mesh_out is NULL");
	if (res3d[0] > 0x7ffffff0u || res3d[1] > 0x7ffffff0u || res3d[2] > 0x7ffffff0u) return fail(NRS_ERR_INVALID_ARG, "nrs_mesh_extract: res3d: 3 * rx * ry * rz reaches 2^31");
	const uint32_t res[3] = {next_multiple_16(res3d[0]), next_multiple_16(res3d[1]), next_multiple_16(res3d[2])}; // :4615-4617
	NRS_TRY(check_lattice(res, aabb_min, aabb_max, thresh, "nrs_mesh_extract"));
	if (!model->have_params) return fail(NRS_ERR_STATE, "nrs_mesh_extract: parameters not set (nrs_model_set_params)");
	HIP_TRY(hipSetDevice(model->ctx->device));
	DeviceBuffer<float> d_density;
	hipError_t he = d_density.alloc((size_t)res[0] * res[1] * res[2]);
	if (he != hipSuccess) return fail_hip(he, "nrs_mesh_extract: device allocation (lattice)");
	NRS_LAUNCH(launch_grid_eval(model->dm, kGridDensity, res, aabb_min, aabb_max, nullptr, mask_with_density_grid ? model->d_density_grid.get() : nullptr, d_density.get(), model->ctx->n_cus,
	                            stream));
	std::unique_ptr<nrs_mesh> mesh;
	NRS_TRY(build_mesh(model->ctx->device, stream, res, aabb_min, aabb_max, thresh, d_density.get(), mesh, "nrs_mesh_extract"));
	// compute_mesh_vertex_colors (:4515-4536): all padded rows, like the reference
	const uint32_t np = mesh->n_padded;
	DeviceBuffer<float> d_coords;
	DeviceBuffer<uint16_t> d_net; // fp16, 16 channels per vertex
	he = mesh->d_colors.alloc((size_t)np * 3);
	if (he == hipSuccess) he = d_coords.alloc((size_t)np * NRS_NETWORK_INPUT_FLOATS);
	if (he == hipSuccess) he = d_net.alloc((size_t)np * NRS_NETWORK_OUTPUT_WIDTH);
	if (he != hipSuccess) return fail_hip(he, "nrs_mesh_extract: device allocation (colours)");
	mesh->has_colors = true;
	if (np) {
		NRS_LAUNCH(launch_mesh_color_inputs(np, mesh->d_verts.get(), model->dm.aabb, d_coords.get(), stream));
		NRS_LAUNCH(launch_network(model->dm, kNetInference, np, d_coords.get(), NRS_NETWORK_INPUT_FLOATS, d_net.get(), NRS_NETWORK_OUTPUT_WIDTH, NRS_INTERLEAVED, model->ctx->n_cus, stream));
		NRS_LAUNCH(launch_mesh_colors(np, d_net.get(), model->dm.rgb_activation, linear_colors, mesh->d_colors.get(), stream));
		HIP_TRY(hipStreamSynchronize((hipStream_t)stream)); // the temporaries go when this returns
	}
	*out = mesh.release();
	return NRS_OK;
}

int nrs_mesh_counts(const nrs_mesh* mesh, uint32_t* n_verts, uint32_t* n_verts_padded, uint32_t* n_tris) {
	if (!mesh) return fail(NRS_ERR_INVALID_ARG, "nrs_mesh_counts: mesh is NULL");
	if (n_verts) *n_verts = mesh->n_verts;
	if (n_verts_padded) *n_verts_padded = mesh->n_padded;
	if (n_tris) *n_tris = mesh->n_tris;
	return NRS_OK;
}

int nrs_mesh_device(const nrs_mesh* mesh, const float** d_verts, const float** d_normals, const float** d_colors, const float** d_smoothed, const uint32_t** d_indices) {
	if (!mesh) return fail(NRS_ERR_INVALID_ARG, "nrs_mesh_device: mesh is NULL");
	if (d_verts) *d_verts = mesh->d_verts.get();
	if (d_normals) *d_normals = mesh->d_normals.get();
	if (d_colors) *d_colors = mesh->has_colors ? mesh->d_colors.get() : nullptr;
	if (d_smoothed) *d_smoothed = mesh->d_smoothed.get();
	if (d_indices) *d_indices = mesh->d_indices.get();
	return NRS_OK;
}

int nrs_mesh_download(const nrs_mesh* mesh, float* h_verts, float* h_normals, float* h_colors, float* h_smoothed, uint32_t* h_indices) {
	if (!mesh) return fail(NRS_ERR_INVALID_ARG, "nrs_mesh_download: mesh is NULL");
	if (h_colors && !mesh->has_colors) return fail(NRS_ERR_STATE, "nrs_mesh_download: h_colors asked of a mesh without colours (nrs_mesh_from_density)");
	HIP_TRY(hipSetDevice(mesh->device));
	const size_t np = mesh->n_padded;
	if (h_verts && np) HIP_TRY(hipMemcpy(h_verts, mesh->d_verts.get(), np * 3 * sizeof(float), hipMemcpyDeviceToHost));
	if (h_normals && np) HIP_TRY(hipMemcpy(h_normals, mesh->d_normals.get(), np * 3 * sizeof(float), hipMemcpyDeviceToHost));
	if (h_colors && np) HIP_TRY(hipMemcpy(h_colors, mesh->d_colors.get(), np * 3 * sizeof(float), hipMemcpyDeviceToHost));
	if (h_smoothed && np) HIP_TRY(hipMemcpy(h_smoothed, mesh->d_smoothed.get(), np * 4 * sizeof(float), hipMemcpyDeviceToHost));
	if (h_indices && mesh->n_tris) HIP_TRY(hipMemcpy(h_indices, mesh->d_indices.get(), (size_t)mesh->n_tris * 3 * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return NRS_OK;
}

void nrs_mesh_destroy(nrs_mesh* mesh) {
	if (!mesh) return;
	(void)hipSetDevice(mesh->device);
	delete mesh;
}

} // extern "C"
