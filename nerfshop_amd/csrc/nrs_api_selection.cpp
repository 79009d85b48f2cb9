// nrs_api_selection.cpp -- the selection tool: region growing on the host (RegionGrowing, region_growing.cu), morphology of a bitfield level on the device with its host
// twin (CorrectMMOperations, correct_mm_operations.cu), and the fine mesh of a selection (GrowingSelection::extract_fine_mesh, growing_selection.cu:2096-2162).
#include "nrs_handles.h"
#include "nrs_selection.h"

#include <cmath>
#include <cstring>

using namespace nrs;

namespace {

constexpr uint32_t kLevelBytes = kGridVol / 8;

// tcnn morton3D / morton3D_invert for coordinates below 128, from tables
struct MortonTables {
	uint32_t spread[kGrid];
	MortonTables() {
		for (uint32_t v = 0; v < kGrid; ++v) {
			uint32_t s = 0;
			for (uint32_t b = 0; b < 7; ++b) s |= ((v >> b) & 1u) << (3 * b);
			spread[v] = s;
		}
	}
};
const MortonTables& tables() {
	static const MortonTables t;
	return t;
}
inline uint32_t morton(uint32_t x, uint32_t y, uint32_t z) {
	const MortonTables& t = tables();
	return t.spread[x] | (t.spread[y] << 1) | (t.spread[z] << 2);
}
inline uint32_t compact(uint32_t m) {
	uint32_t v = 0;
	for (uint32_t b = 0; b < 7; ++b) v |= ((m >> (3 * b)) & 1u) << b;
	return v;
}
struct Cell { uint32_t x, y, z; };
inline Cell cell_of(uint32_t pos_idx) { return {compact(pos_idx), compact(pos_idx >> 1), compact(pos_idx >> 2)}; }
inline bool on_shell(const Cell& c) { // is_boundary, selection_utils.cu:8-13
	return c.x == 0 || c.y == 0 || c.z == 0 || c.x == kGrid - 1 || c.y == kGrid - 1 || c.z == kGrid - 1;
}
inline bool get_bit(const std::vector<uint8_t>& bits, uint32_t cell) { return (bits[cell / 8] >> (cell % 8)) & 1u; }
inline void set_bit(std::vector<uint8_t>& bits, uint32_t cell) { bits[cell / 8] |= (uint8_t)(1u << (cell % 8)); }

// upscale_selection, region_growing.cu:57-91
void upscale(nrs_selection& s) {
	if (s.level == s.max_cascade || s.level + 1 >= kCascades) return;
	s.level += 1;
	std::fill(s.bits.begin(), s.bits.end(), 0);
	for (uint32_t& cell : s.cells) {
		cell = nrs_upper_cell_idx(cell, s.level);
		set_bit(s.bits, cell);
	}
	for (uint32_t& cell : s.queue) cell = nrs_upper_cell_idx(cell, s.level);
}

// L from S at the growing level in the loop order of CorrectMMOperations::dilate / erode (x outer, y, z inner: correct_mm_operations.cu:135-148)
void cells_from_bits(nrs_selection& s) {
	s.cells.clear();
	const uint32_t first = s.level * kGridVol;
	for (uint32_t x = 0; x < kGrid; ++x)
		for (uint32_t y = 0; y < kGrid; ++y)
			for (uint32_t z = 0; z < kGrid; ++z) {
				const uint32_t cell = first + morton(x, y, z);
				if (get_bit(s.bits, cell)) s.cells.push_back(cell);
			}
}

const char* check_element(int se_type, int radius) {
	if (se_type != NRS_SE_CUBE && se_type != NRS_SE_SPHERE) return "se_type is neither NRS_SE_CUBE nor NRS_SE_SPHERE";
	if (radius < 1 || radius > kMorphMaxRadius) return "radius is outside 1..10";
	return nullptr;
}
// x half-width of the element's row (dy, dz), -1 when the row is not part of it
int row_half_width(int se_type, int r, int dy, int dz) {
	if (se_type == NRS_SE_CUBE) return r;
	const int rest = r * r - dy * dy - dz * dz;
	if (rest < 0) return -1;
	int h = 0;
	while ((h + 1) * (h + 1) <= rest) ++h;
	return h;
}
MorphPlan make_plan(int op, int se_type, int r) {
	MorphPlan p{};
	p.invert = op == NRS_MORPH_ERODE;
	for (int h = r; h >= 0; --h)
		for (int dz = -r; dz <= r; ++dz)
			for (int dy = -r; dy <= r; ++dy)
				if (row_half_width(se_type, r, dy, dz) == h) {
					p.dy[p.n_taps] = (int8_t)dy;
					p.dz[p.n_taps] = (int8_t)dz;
					p.half[p.n_taps++] = (int8_t)h;
				}
	return p;
}

int check_morph_args(const void* in, uint32_t level, int op, int se_type, int radius, const void* out, const char* fn, const char* in_name, const char* out_name) {
	const std::string f = std::string(fn) + ": ";
	if (!in) return fail(NRS_ERR_INVALID_ARG, f + in_name + " is NULL");
	if (!out) return fail(NRS_ERR_INVALID_ARG, f + out_name + " is NULL");
	if (level >= kCascades) return fail(NRS_ERR_INVALID_ARG, f + "level is above 4");
	if (op != NRS_MORPH_DILATE && op != NRS_MORPH_ERODE) return fail(NRS_ERR_INVALID_ARG, f + "op is neither NRS_MORPH_DILATE nor NRS_MORPH_ERODE");
	if (const char* what = check_element(se_type, radius)) return fail(NRS_ERR_INVALID_ARG, f + what);
	const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out;
	if (a < b + NRS_BITFIELD_BYTES && b < a + NRS_BITFIELD_BYTES) return fail(NRS_ERR_INVALID_ARG, f + out_name + " overlaps " + in_name);
	return NRS_OK;
}

// the handle's device buffers, on the context's device
int device_state(nrs_ctx* ctx, nrs_selection* sel, const char* fn) {
	if (sel->device >= 0 && sel->device != ctx->device) return fail(NRS_ERR_INVALID_ARG, std::string(fn) + ": ctx is on another device than the selection's buffers");
	HIP_TRY(hipSetDevice(ctx->device));
	if (sel->device < 0) {
		hipError_t he = sel->d_work.alloc(3 * (size_t)kMorphLevelWords);
		if (he == hipSuccess) he = sel->d_lattice.alloc(kGridVol);
		if (he != hipSuccess) {
			sel->d_work.reset();
			return fail_hip(he, (std::string(fn) + ": device allocation").c_str());
		}
		sel->device = ctx->device;
	}
	return NRS_OK;
}
uint32_t* d_morton(nrs_selection* sel) { return sel->d_work.get(); }
uint32_t* d_rows(nrs_selection* sel, int k) { return sel->d_work.get() + (size_t)(1 + k) * kMorphLevelWords; }

// the growing level of S to the device, as rows in d_rows(0)
int upload_rows(nrs_selection* sel, hipStream_t s) {
	HIP_TRY(hipMemcpyAsync(d_morton(sel), sel->bits.data() + (size_t)sel->level * kLevelBytes, kLevelBytes, hipMemcpyHostToDevice, s));
	NRS_LAUNCH(launch_morph_pack(d_morton(sel), d_rows(sel, 0), s));
	return NRS_OK;
}
// d_rows(k) becomes S (the other levels zero, like the vector the reference starts from) and L; synchronises
int download_rows(nrs_selection* sel, int k, hipStream_t s) {
	NRS_LAUNCH(launch_morph_unpack(d_rows(sel, k), d_morton(sel), s));
	HIP_TRY(hipStreamSynchronize(s)); // upload_rows' copy out of `bits` has been made before they are cleared
	std::fill(sel->bits.begin(), sel->bits.end(), 0);
	HIP_TRY(hipMemcpyAsync(sel->bits.data() + (size_t)sel->level * kLevelBytes, d_morton(sel), kLevelBytes, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	cells_from_bits(*sel);
	return NRS_OK;
}

int morph_selection(nrs_ctx* ctx, void* stream, nrs_selection* sel, int op, const char* fn) {
	if (!ctx) return fail(NRS_ERR_INVALID_ARG, std::string(fn) + ": ctx is NULL");
	if (!sel) return fail(NRS_ERR_INVALID_ARG, std::string(fn) + ": sel is NULL");
	NRS_TRY(device_state(ctx, sel, fn));
	hipStream_t s = (hipStream_t)stream;
	const MorphPlan plan = op == NRS_MORPH_DILATE ? make_plan(op, sel->dilation_type, sel->dilation_radius) : make_plan(op, sel->erosion_type, sel->erosion_radius);
	NRS_TRY(upload_rows(sel, s));
	NRS_LAUNCH(launch_morph_rows(plan, d_rows(sel, 0), d_rows(sel, 1), s));
	return download_rows(sel, 1, s);
}

} // namespace

extern "C" {

int nrs_selection_create(const float* h_density_grid, size_t n_floats, uint32_t max_cascade, nrs_selection** out) {
	if (!h_density_grid) return fail(NRS_ERR_INVALID_ARG, "nrs_selection_create: h_density_grid is NULL");
	if (!out) return fail(NRS_ERR_INVALID_ARG, "nrs_selection_create: sel_out is NULL");
	if (n_floats != (size_t)kCascades * kGridVol) return fail(NRS_ERR_INVALID_ARG, "nrs_selection_create: n_floats is not 5 * 128^3");
	if (max_cascade >= kCascades) return fail(NRS_ERR_INVALID_ARG, "nrs_selection_create: max_cascade is above 4");
	nrs_selection* sel = new nrs_selection();
	sel->grid.assign(h_density_grid, h_density_grid + n_floats);
	sel->max_cascade = max_cascade;
	sel->bits.assign(NRS_BITFIELD_BYTES, 0);
	*out = sel;
	return NRS_OK;
}

void nrs_selection_destroy(nrs_selection* sel) {
	if (!sel) return;
	if (sel->device >= 0) (void)hipSetDevice(sel->device);
	delete sel;
}

int nrs_selection_reset(nrs_selection* sel, const uint32_t* h_cells, uint32_t n, uint32_t growing_level) {
	if (!sel) return fail(NRS_ERR_INVALID_ARG, "nrs_selection_reset: sel is NULL");
	if (n && !h_cells) return fail(NRS_ERR_INVALID_ARG, "nrs_selection_reset: h_cells is NULL");
	if (growing_level >= kCascades) return fail(NRS_ERR_INVALID_ARG, "nrs_selection_reset: growing_level is above 4");
	for (uint32_t i = 0; i < n; ++i)
		if (h_cells[i] >= kCascades * kGridVol) return fail(NRS_ERR_INVALID_ARG, "nrs_selection_reset: h_cells[" + std::to_string(i) + "] is not a cell of the grid");
	std::fill(sel->bits.begin(), sel->bits.end(), 0);
	sel->queue.clear();
	sel->cells.clear();
	for (uint32_t i = 0; i < n; ++i) {
		uint32_t cell = h_cells[i];
		const uint32_t level = cell / kGridVol;
		if (level > growing_level) continue;
		if (level < growing_level) cell = nrs_upper_cell_idx(cell, growing_level);
		sel->queue.push_back(cell);
		sel->cells.push_back(cell);
	}
	sel->level = growing_level; // not in the reference, which leaves m_growing_level to the grow_region that follows (include/nrs.h says so)
	sel->performed_closing = false;
	return NRS_OK;
}

int nrs_selection_grow(nrs_selection* sel, float density_threshold, uint32_t growing_level, uint32_t growing_steps, uint32_t* n_popped) {
	if (!sel) return fail(NRS_ERR_INVALID_ARG, "nrs_selection_grow: sel is NULL");
	if (!std::isfinite(density_threshold)) return fail(NRS_ERR_INVALID_ARG, "nrs_selection_grow: density_threshold is not finite");
	if (growing_level >= kCascades) return fail(NRS_ERR_INVALID_ARG, "nrs_selection_grow: growing_level is above 4");
	if (n_popped) *n_popped = 0;
	if (sel->queue.empty()) return NRS_OK;
	sel->level = growing_level;
	sel->performed_closing = false;
	uint32_t popped = 0;
	while (!sel->queue.empty() && popped < growing_steps) {
		uint32_t cell = sel->queue.front();
		sel->queue.pop_front();
		++popped;
		uint32_t level = cell / kGridVol;
		if (get_bit(sel->bits, cell) || !(sel->grid[cell] >= density_threshold) || level != sel->level) continue;
		Cell c = cell_of(cell % kGridVol);
		if (on_shell(c)) {
			upscale(*sel);
			cell = nrs_upper_cell_idx(cell, sel->level);
			level = cell / kGridVol;
			c = cell_of(cell % kGridVol);
		}
		const uint32_t first = level * kGridVol;
		if (c.x > 0) sel->queue.push_back(first + morton(c.x - 1, c.y, c.z));
		if (c.y > 0) sel->queue.push_back(first + morton(c.x, c.y - 1, c.z));
		if (c.z > 0) sel->queue.push_back(first + morton(c.x, c.y, c.z - 1));
		if (c.x < kGrid - 1) sel->queue.push_back(first + morton(c.x + 1, c.y, c.z));
		if (c.y < kGrid - 1) sel->queue.push_back(first + morton(c.x, c.y + 1, c.z));
		if (c.z < kGrid - 1) sel->queue.push_back(first + morton(c.x, c.y, c.z + 1));
		sel->cells.push_back(cell);
		set_bit(sel->bits, cell);
	}
	if (n_popped) *n_popped = popped;
	return NRS_OK;
}

int nrs_selection_upscale(nrs_selection* sel) {
	if (!sel) return fail(NRS_ERR_INVALID_ARG, "nrs_selection_upscale: sel is NULL");
	upscale(*sel);
	return NRS_OK;
}

int nrs_selection_state(const nrs_selection* sel, uint32_t* growing_level, uint32_t* n_cells, uint32_t* n_queue, int* performed_closing) {
	if (!sel) return fail(NRS_ERR_INVALID_ARG, "nrs_selection_state: sel is NULL");
	if (growing_level) *growing_level = sel->level;
	if (n_cells) *n_cells = (uint32_t)sel->cells.size();
	if (n_queue) *n_queue = (uint32_t)sel->queue.size();
	if (performed_closing) *performed_closing = sel->performed_closing ? 1 : 0;
	return NRS_OK;
}

int nrs_selection_get_cells(const nrs_selection* sel, uint32_t* h_cells_out, float* h_points_out) {
	if (!sel) return fail(NRS_ERR_INVALID_ARG, "nrs_selection_get_cells: sel is NULL");
	if (h_cells_out && !sel->cells.empty()) memcpy(h_cells_out, sel->cells.data(), sel->cells.size() * sizeof(uint32_t));
	if (h_points_out)
		for (size_t i = 0; i < sel->cells.size(); ++i) { // get_cell_pos, selection_utils.cu:65-68
			const Cell c = cell_of(sel->cells[i] % kGridVol);
			const float scale = std::scalbn(1.0f, (int)(sel->cells[i] / kGridVol));
			const uint32_t xyz[3] = {c.x, c.y, c.z};
			for (int k = 0; k < 3; ++k) h_points_out[3 * i + k] = (((float)xyz[k] + 0.5f) / (float)kGrid - 0.5f) * scale + 0.5f;
		}
	return NRS_OK;
}

int nrs_selection_get_bitfield(const nrs_selection* sel, uint8_t* h_bitfield_out) {
	if (!sel) return fail(NRS_ERR_INVALID_ARG, "nrs_selection_get_bitfield: sel is NULL");
	if (!h_bitfield_out) return fail(NRS_ERR_INVALID_ARG, "nrs_selection_get_bitfield: h_bitfield_out is NULL");
	memcpy(h_bitfield_out, sel->bits.data(), NRS_BITFIELD_BYTES);
	return NRS_OK;
}

int nrs_selection_set_structuring_elements(nrs_selection* sel, int dilation_type, int dilation_radius, int erosion_type, int erosion_radius) {
	if (!sel) return fail(NRS_ERR_INVALID_ARG, "nrs_selection_set_structuring_elements: sel is NULL");
	if (const char* what = check_element(dilation_type, dilation_radius)) return fail(NRS_ERR_INVALID_ARG, std::string("nrs_selection_set_structuring_elements: dilation: ") + what);
	if (const char* what = check_element(erosion_type, erosion_radius)) return fail(NRS_ERR_INVALID_ARG, std::string("nrs_selection_set_structuring_elements: erosion: ") + what);
	sel->dilation_type = dilation_type;
	sel->dilation_radius = dilation_radius;
	sel->erosion_type = erosion_type;
	sel->erosion_radius = erosion_radius;
	return NRS_OK;
}

int nrs_bitfield_morph_host(const uint8_t* h_in, uint32_t level, int op, int se_type, int radius, uint8_t* h_out) {
	NRS_TRY(check_morph_args(h_in, level, op, se_type, radius, h_out, "nrs_bitfield_morph_host", "h_in", "h_out"));
	// the level unpacked to a byte per cell, z fastest like the reference's loops, so that a tap is a load and not a Morton encode
	std::vector<uint8_t> cells(kGridVol);
	const uint8_t* in = h_in + (size_t)level * kLevelBytes;
	for (uint32_t x = 0; x < kGrid; ++x)
		for (uint32_t y = 0; y < kGrid; ++y)
			for (uint32_t z = 0; z < kGrid; ++z) {
				const uint32_t m = morton(x, y, z);
				cells[(x * kGrid + y) * kGrid + z] = (in[m / 8] >> (m % 8)) & 1u;
			}
	// the element's support (SphereSE::update_support; CubeSE's three loops) as its (i, j) columns: the k of a column are a run, clipped to the grid per cell
	struct Column { int i, j, h; };
	std::vector<Column> support;
	for (int i = -radius; i <= radius; ++i)
		for (int j = -radius; j <= radius; ++j) {
			const int h = row_half_width(se_type, radius, i, j);
			if (h >= 0) support.push_back({i, j, h});
		}
	memset(h_out, 0, NRS_BITFIELD_BYTES);
	uint8_t* out = h_out + (size_t)level * kLevelBytes;
	const uint8_t stop_at = op == NRS_MORPH_DILATE ? 1 : 0; // hit ends at the first set tap, fit at the first clear one
	// (x, y) columns of the grid that hold such a cell at all: the others are passed over without a look at their taps
	std::vector<uint8_t> worth(kGrid * kGrid, 0);
	for (uint32_t c = 0; c < kGridVol; ++c)
		if (cells[c] == stop_at) worth[c / kGrid] = 1;
	const int n = (int)kGrid;
	for (int x = 0; x < n; ++x)
		for (int y = 0; y < n; ++y)
			for (int z = 0; z < n; ++z) {
				bool stopped = false;
				for (const Column& t : support) {
					const int a = x + t.i, b = y + t.j;
					if (a < 0 || b < 0 || a >= n || b >= n || !worth[(size_t)a * n + b]) continue; // in_grid
					const uint8_t* column = cells.data() + ((size_t)a * n + b) * n;
					for (int c = std::max(z - t.h, 0), last = std::min(z + t.h, n - 1); c <= last && !stopped; ++c) stopped = column[c] == stop_at;
					if (stopped) break;
				}
				if (stopped == (op == NRS_MORPH_DILATE)) {
					const uint32_t m = morton((uint32_t)x, (uint32_t)y, (uint32_t)z);
					out[m / 8] |= (uint8_t)(1u << (m % 8));
				}
			}
	return NRS_OK;
}

int nrs_bitfield_morph(nrs_ctx* ctx, void* stream, const uint8_t* d_in, uint32_t level, int op, int se_type, int radius, uint8_t* d_out) {
	if (!ctx) return fail(NRS_ERR_INVALID_ARG, "nrs_bitfield_morph: ctx is NULL");
	NRS_TRY(check_morph_args(d_in, level, op, se_type, radius, d_out, "nrs_bitfield_morph", "d_in", "d_out"));
	if ((uintptr_t)d_in % 16) return fail(NRS_ERR_INVALID_ARG, "nrs_bitfield_morph: d_in is not 16-byte aligned");
	if ((uintptr_t)d_out % 16) return fail(NRS_ERR_INVALID_ARG, "nrs_bitfield_morph: d_out is not 16-byte aligned");
	HIP_TRY(hipSetDevice(ctx->device));
	hipStream_t s = (hipStream_t)stream;
	// two of d_out's other levels hold the rows until the memsets that leave them zero
	uint32_t* out_levels = reinterpret_cast<uint32_t*>(d_out);
	uint32_t* rows_in = out_levels + (size_t)((level + 1) % kCascades) * kMorphLevelWords;
	uint32_t* rows_out = out_levels + (size_t)((level + 2) % kCascades) * kMorphLevelWords;
	NRS_LAUNCH(launch_morph_pack(reinterpret_cast<const uint32_t*>(d_in) + (size_t)level * kMorphLevelWords, rows_in, s));
	NRS_LAUNCH(launch_morph_rows(make_plan(op, se_type, radius), rows_in, rows_out, s));
	NRS_LAUNCH(launch_morph_unpack(rows_out, out_levels + (size_t)level * kMorphLevelWords, s));
	if (level > 0) HIP_TRY(hipMemsetAsync(d_out, 0, (size_t)level * kLevelBytes, s));
	if (level + 1 < kCascades) HIP_TRY(hipMemsetAsync(d_out + (size_t)(level + 1) * kLevelBytes, 0, (size_t)(kCascades - 1 - level) * kLevelBytes, s));
	return NRS_OK;
}

int nrs_selection_dilate(nrs_ctx* ctx, void* stream, nrs_selection* sel) { return morph_selection(ctx, stream, sel, NRS_MORPH_DILATE, "nrs_selection_dilate"); }
int nrs_selection_erode(nrs_ctx* ctx, void* stream, nrs_selection* sel) { return morph_selection(ctx, stream, sel, NRS_MORPH_ERODE, "nrs_selection_erode"); }

int nrs_selection_fine_mesh(nrs_ctx* ctx, void* stream, nrs_selection* sel, int use_morphological, nrs_mesh** out) {
	if (!ctx) return fail(NRS_ERR_INVALID_ARG, "nrs_selection_fine_mesh: ctx is NULL");
	if (!sel) return fail(NRS_ERR_INVALID_ARG, "nrs_selection_fine_mesh: sel is NULL");
	if (!out) return fail(NRS_ERR_INVALID_ARG, "nrs_selection_fine_mesh: mesh_out is NULL");
	NRS_TRY(device_state(ctx, sel, "nrs_selection_fine_mesh"));
	hipStream_t s = (hipStream_t)stream;
	if (use_morphological && !sel->performed_closing) {
		// dilate, erode: S -> rows 0 -> rows 1 -> rows 0, and the lattice is cut from rows 0 where they lie; the copy back to the host only refreshes S and L
		NRS_TRY(upload_rows(sel, s));
		NRS_LAUNCH(launch_morph_rows(make_plan(NRS_MORPH_DILATE, sel->dilation_type, sel->dilation_radius), d_rows(sel, 0), d_rows(sel, 1), s));
		NRS_LAUNCH(launch_morph_rows(make_plan(NRS_MORPH_ERODE, sel->erosion_type, sel->erosion_radius), d_rows(sel, 1), d_rows(sel, 0), s));
		NRS_LAUNCH(launch_selection_lattice(d_rows(sel, 0), sel->d_lattice.get(), s));
		NRS_TRY(download_rows(sel, 0, s));
		sel->performed_closing = true;
	} else {
		// the cells of L at the growing level as rows (the shell is left out by the kernel)
		std::vector<uint32_t> rows(kMorphLevelWords, 0u);
		for (const uint32_t cell : sel->cells) {
			if (cell / kGridVol != sel->level) continue;
			const Cell c = cell_of(cell % kGridVol);
			rows[(c.z * kGrid + c.y) * 4u + c.x / 32u] |= 1u << (c.x % 32u);
		}
		HIP_TRY(hipMemcpyAsync(d_rows(sel, 0), rows.data(), kLevelBytes, hipMemcpyHostToDevice, s));
		NRS_LAUNCH(launch_selection_lattice(d_rows(sel, 0), sel->d_lattice.get(), s));
		HIP_TRY(hipStreamSynchronize(s)); // `rows` goes when this block ends
	}
	const float scale = std::scalbn(1.0f, (int)sel->level); // :2109-2112
	const float mn = scale * (0.f - 0.5f) + 0.5f, mx = scale * (1.f - 0.5f) + 0.5f;
	const uint32_t res3d[3] = {kGrid, kGrid, kGrid};
	const float aabb_min[3] = {mn, mn, mn}, aabb_max[3] = {mx, mx, mx};
	return mesh_from_lattice(ctx->device, stream, res3d, aabb_min, aabb_max, 0.5f, sel->d_lattice.get(), out, "nrs_selection_fine_mesh");
}

} // extern "C"
