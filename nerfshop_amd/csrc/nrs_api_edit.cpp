// nrs_api_edit.cpp -- the edit operators: cage (tet LUT, fine look-up table, per-move updates, membrane terms) and affine duplication.
#include "nrs_host.h"
#include "nrs_tables.h"
#include "nrs_cage.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <new>

using namespace nrs;

static void box_of(const float* v, uint32_t n, Box3& b) {
	const float inf = std::numeric_limits<float>::infinity();
	for (int k = 0; k < 3; ++k) { b.mn[k] = inf; b.mx[k] = -inf; }
	for (uint32_t i = 0; i < n; ++i)
		for (int k = 0; k < 3; ++k) {
			b.mn[k] = std::fmin(b.mn[k], v[3 * i + k]);
			b.mx[k] = std::fmax(b.mx[k], v[3 * i + k]);
		}
}
static void warp_box(const Box3& b, const Box3& aabb, Box3& out) { // BoundingBox::warp_box, bounding_box.cuh:272
	for (int k = 0; k < 3; ++k) {
		const float diag = aabb.mx[k] - aabb.mn[k];
		out.mn[k] = (b.mn[k] - aabb.mn[k]) / diag;
		out.mx[k] = (b.mx[k] - aabb.mn[k]) / diag;
	}
}

template <typename T>
static int upload(DeviceBuffer<T>& buf, const T* h, size_t count) {
	HIP_TRY(buf.alloc(count));
	if (count) HIP_TRY(hipMemcpy(buf.get(), h, count * sizeof(T), hipMemcpyHostToDevice));
	return NRS_OK;
}

// ---- edit operators ------------------------------------------------------------------------------------------------
// ---- device-side tet LUT (nrs_cage.hip) ------------------------------------------------------------------------------
static int ensure_build_scratch(nrs_edit* e) {
	const size_t n_cells = (size_t)kGridVol * kCascades;
	if (!e->d_counts.get()) {
		HIP_TRY(e->d_counts.alloc(n_cells));
		HIP_TRY(hipMemset(e->d_counts.get(), 0, n_cells * 4));
	}
	if (!e->d_tile_sums.get()) HIP_TRY(e->d_tile_sums.alloc(kLutScanTiles));
	if (!e->d_hit_masks.get()) HIP_TRY(e->d_hit_masks.alloc((size_t)e->n_tets * kCascades * 2));
	if (!e->d_scratch.get()) HIP_TRY(e->d_scratch.alloc(16));
	return NRS_OK;
}
// cell -> tet CSR of `d_verts` into e->d_lut_off / e->d_lut_idx (grown as needed); optionally the touched-cell bitfield.
// Synchronises the stream once (the entry count decides the idx allocation), like the reference's host builder does.
static int build_lut_on_device(nrs_edit* e, const float* d_verts, uint8_t* d_bitfield_out, hipStream_t s) {
	NRS_TRY(ensure_build_scratch(e));
	// cells of cascade 0 in an average tet's bounding box, from the mesh's box and tet count (six tets share a lattice cube's box): only the kernels' team size hangs on it
	float cells0 = 0.f;
	{
		const Box3& bb = e->de.bbox;
		const double vol = (double)std::max(bb.mx[0] - bb.mn[0], 0.f) * std::max(bb.mx[1] - bb.mn[1], 0.f) * std::max(bb.mx[2] - bb.mn[2], 0.f);
		const double side = std::cbrt(vol / std::max<double>(e->n_tets / 6.0, 1.0)) * kGrid;
		cells0 = (float)((side + 1.0) * (side + 1.0) * (side + 1.0));
	}
	NRS_LAUNCH(launch_lut_count_scan(e->n_tets, d_verts, e->de.tets, e->d_counts.get(), e->d_tile_sums.get(), e->d_lut_off.get(), e->d_scratch.get() + 6, e->d_hit_masks.get(), cells0, s));
	uint32_t total = 0;
	HIP_TRY(hipMemcpyAsync(&total, e->d_scratch.get() + 6, 4, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	if ((size_t)total > e->lut_idx_cap || !e->d_big_cells.get()) {
		const size_t cap = std::max<size_t>((size_t)total + total / 2, 1024);
		DeviceBuffer<uint32_t> fresh, fresh_big; // (a failed growth leaves the operator its old, valid table)
		HIP_TRY(fresh.alloc(cap));
		HIP_TRY(fresh_big.alloc(lut_big_list_capacity(cap)));
		e->d_lut_idx = std::move(fresh);
		e->d_big_cells = std::move(fresh_big);
		e->lut_idx_cap = cap;
		e->de.lut_idx = e->d_lut_idx.get();
	}
	NRS_LAUNCH(launch_lut_fill(e->n_tets, d_verts, e->de.tets, e->d_counts.get(), e->d_lut_off.get(), e->d_lut_idx.get(), d_bitfield_out, e->d_scratch.get() + 7, e->d_big_cells.get(), lut_big_list_capacity(e->lut_idx_cap), e->d_hit_masks.get(), cells0, s));
	e->lut_n_idx = total;
	return NRS_OK;
}
// The fine look-up table of e's CURRENT LUT and plane records (both on the device, written on stream s): DeviceEdit::fine_*.  Leaves the operator without one (the kernels
// then scan the LUT's own lists) when the mesh reaches no cell, when even one fine cell per LUT cell would exceed kFineMaxCells, or when NRS_NO_FINE_LUT is set (A/B).
// The table comes with a head word per fine cell (DeviceEdit::fine_head) unless a tet number would not fit its 25 bits or NRS_NO_FINE_HEAD is set (A/B, and the test
// of that fallback); a fine list is a filtered LUT list of a cascade that passed kFineMaxList, so its length always fits the head's 7 bits.
// Two small read-backs (the window, the entry count), like the LUT's own build.
int nrs::build_fine_lut(nrs_edit* e, hipStream_t s) {
	static const bool off = dev_knob("NRS_NO_FINE_LUT") != nullptr;
	static const bool no_head = dev_knob("NRS_NO_FINE_HEAD") != nullptr;
	const bool want_head = !no_head && e->n_tets < (1u << kFineHeadTetBits);
	DeviceEdit& de = e->de;
	de.fine_off = nullptr;
	de.fine_idx = nullptr;
	de.fine_head = nullptr;
	memset(de.fine_win, 0, sizeof(de.fine_win));
	e->fine_n_idx = 0;
	if (off) return NRS_OK;
	if (!e->d_fine_win.get()) HIP_TRY(e->d_fine_win.alloc(kCascades * 8 + 8));
	if (!e->d_fine_tiles.get()) HIP_TRY(e->d_fine_tiles.alloc(kFineScanTiles));
	NRS_LAUNCH(launch_fine_window(de.lut_off, e->d_fine_win.get(), s));
	int32_t win[kCascades * 8];
	HIP_TRY(hipMemcpyAsync(win, e->d_fine_win.get(), sizeof(win), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	// per cascade, finest first: 4 x 4 x 4 fine cells per LUT cell while the budget lasts (then 2 x 2 x 2, then none); a cascade whose longest list is a mesh-in-a-cell
	// (thousands of tets: the coarse cascades of a small cage) keeps the LUT's own lists -- the scene's samples hardly stand there and the build would walk them 64 times
	uint64_t budget = kFineMaxCells;
	uint32_t base = 0;
	bool any = false;
	for (uint32_t c = 0; c < kCascades; ++c) {
		const int32_t* w = win + 8 * c;
		int32_t* f = de.fine_win[c];
		f[3] = (int32_t)base;
		f[7] = kFinePlain;
		if (w[0] > w[3]) { f[7] = 0; continue; } // no tet reaches this cascade: extent 0, every look-up finds nothing (as the LUT's empty lists say)
		if (w[7] > kFineMaxList) continue;
		for (int shift = 2; shift >= 1; --shift) {
			const uint64_t cells = ((uint64_t)(w[3] - w[0] + 1) << shift) * ((uint64_t)(w[4] - w[1] + 1) << shift) * ((uint64_t)(w[5] - w[2] + 1) << shift);
			if (cells > budget) continue;
			for (int a = 0; a < 3; ++a) { f[a] = w[a] << shift; f[4 + a] = (w[3 + a] - w[a] + 1) << shift; }
			f[7] = shift;
			budget -= cells;
			base += (uint32_t)cells;
			any = true;
			break;
		}
	}
	if (!any) { memset(de.fine_win, 0, sizeof(de.fine_win)); return NRS_OK; }
	const uint32_t n_cells = base, n_padded = (n_cells + 4095u) / 4096u * 4096u;
	if (n_padded > e->fine_cells_cap || (want_head && !e->d_fine_head.get())) {
		e->d_fine_off.reset(); e->d_fine_counts.reset(); e->d_fine_head.reset();
		e->fine_cells_cap = 0;
		const size_t cap = std::min<size_t>(kFineMaxCells, (size_t)n_padded + n_padded / 4 + 4095) / 4096 * 4096;
		HIP_TRY(e->d_fine_off.alloc(cap + 1));
		HIP_TRY(e->d_fine_counts.alloc(cap));
		if (want_head) HIP_TRY(e->d_fine_head.alloc(cap)); // (a refusal: no fine table at all, like a refusal of the offsets -- de.fine_* are null already)
		e->fine_cells_cap = cap;
	}
	NRS_LAUNCH(launch_fine_count_scan(de, n_cells, e->d_fine_counts.get(), e->d_fine_tiles.get(), e->d_fine_off.get(), (uint32_t*)e->d_fine_win.get() + kCascades * 8, s));
	uint32_t n_idx = 0;
	HIP_TRY(hipMemcpyAsync(&n_idx, e->d_fine_win.get() + kCascades * 8, 4, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	if ((size_t)n_idx > e->fine_idx_cap || !e->d_fine_idx.get()) {
		e->d_fine_idx.reset();
		e->fine_idx_cap = 0;
		const size_t cap = std::max<size_t>((size_t)n_idx + n_idx / 2, 1024);
		HIP_TRY(e->d_fine_idx.alloc(cap));
		e->fine_idx_cap = cap;
	}
	NRS_LAUNCH(launch_fine_fill(de, n_cells, e->d_fine_off.get(), e->d_fine_idx.get(), want_head ? e->d_fine_head.get() : nullptr, s));
	e->fine_n_idx = n_idx;
	de.fine_off = e->d_fine_off.get();
	de.fine_idx = e->d_fine_idx.get();
	de.fine_head = want_head ? e->d_fine_head.get() : nullptr;
	static const bool log_fine = dev_knob("NRS_FINE_LOG") != nullptr;
	if (log_fine) fprintf(stderr, "[nrs fine lut] %u fine cells, %u entries (the LUT holds %u), subdivision per cascade %d %d %d %d %d, head words %s\n", n_cells, n_idx, e->lut_n_idx, de.fine_win[0][7],
	                      de.fine_win[1][7], de.fine_win[2][7], de.fine_win[3][7], de.fine_win[4][7], de.fine_head ? "yes" : "no");
	return NRS_OK;
}
// everything that follows new deformed vertices in e->d_verts: bbox, LUT, rotations.  Synchronous.
static int rebuild_after_vertices(nrs_edit* e, hipStream_t s, bool build_fine_now = false) {
	NRS_TRY(ensure_build_scratch(e));
	NRS_LAUNCH(launch_bbox(e->n_vertices, e->d_verts.get(), (float*)e->d_scratch.get(), s));
	NRS_TRY(build_lut_on_device(e, e->d_verts.get(), nullptr, s));
	// (the rotation of a tet's map-back record and its plane record: both of the new pose, on this stream, before the next reader)
	if (e->d_rot.get()) NRS_LAUNCH(launch_local_rotations(e->n_tets, e->d_verts.get(), e->de.orig, e->de.tets, e->d_rot.get(), e->d_mapback.get(), s));
	NRS_LAUNCH(launch_tet_planes(e->n_tets, e->d_verts.get(), e->de.tets, e->d_planes.get(), s));
	if (build_fine_now) NRS_TRY(build_fine_lut(e, s));
	else { // (see nrs_edit::fine_stale)
		e->de.fine_off = nullptr;
		e->de.fine_idx = nullptr;
		e->de.fine_head = nullptr;
		memset(e->de.fine_win, 0, sizeof(e->de.fine_win));
		e->fine_stale = true;
		e->renders_since_move = 0;
	}
	uint32_t host[8];
	HIP_TRY(hipMemcpyAsync(host, e->d_scratch.get(), sizeof(host), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	memcpy(e->de.bbox.mn, host, 12);      // post_update_vertices, tet_mesh.cu:12-20
	memcpy(e->de.bbox.mx, host + 3, 12);
	warp_box(e->de.bbox, e->de.aabb, e->de.warped_bbox);
	e->lut_max_per_cell = host[7];
	return NRS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
extern "C" {

int nrs_edit_create(nrs_ctx* ctx, const nrs_model_desc* desc, const nrs_tet_mesh* mesh, nrs_edit** out) {
	if (!ctx || !desc || !mesh || !out) return fail(NRS_ERR_INVALID_ARG, "nrs_edit_create: NULL argument");
	if (!mesh->h_vertices || !mesh->h_original_vertices || !mesh->h_tets) return fail(NRS_ERR_INVALID_ARG, "nrs_edit_create: missing mesh array");
	if (mesh->n_tets == 0 || mesh->n_vertices == 0) return fail(NRS_ERR_INVALID_ARG, "nrs_edit_create: empty mesh");
	if (mesh->apply_poisson && (!mesh->h_boundary_shs || !mesh->h_boundary_outside_density || !mesh->h_boundary_residual_density))
		return fail(NRS_ERR_INVALID_ARG, "nrs_edit_create: apply_poisson set without the per-vertex membrane arrays");
	for (size_t i = 0; i < 4 * (size_t)mesh->n_tets; ++i)
		if (mesh->h_tets[i] >= mesh->n_vertices) return fail(NRS_ERR_INVALID_ARG, "nrs_edit_create: tet index out of range");
	const size_t n_cells = (size_t)kGridVol * kCascades;
	const bool host_lut = mesh->h_lut_offsets != nullptr;
	const uint32_t n_idx = host_lut ? mesh->h_lut_offsets[n_cells] : 0;
	if (n_idx && !mesh->h_lut_idx) return fail(NRS_ERR_INVALID_ARG, "nrs_edit_create: h_lut_idx is NULL");
	HIP_TRY(hipSetDevice(ctx->device));
	std::unique_ptr<nrs_edit> owner(new (std::nothrow) nrs_edit()); // (a refusal below takes the operator and its buffers with it)
	nrs_edit* e = owner.get();
	if (!e) return fail(NRS_ERR_STATE, "out of host memory");
	e->ctx = ctx;
	e->n_vertices = mesh->n_vertices;
	e->n_tets = mesh->n_tets;
	DeviceEdit& de = e->de;
	for (int k = 0; k < 3; ++k) { de.aabb.mn[k] = desc->aabb_min[k]; de.aabb.mx[k] = desc->aabb_max[k]; }
	de.diag_pow2 = 1;
	for (int k = 0; k < 3; ++k) {
		const float diag = desc->aabb_max[k] - desc->aabb_min[k];
		int ex = 0;
		if (std::frexp(diag, &ex) != 0.5f) de.diag_pow2 = 0;
		de.inv_diag[k] = 1.0f / diag;
	}
	Box3 orig_bbox;
	box_of(mesh->h_vertices, mesh->n_vertices, de.bbox);           // post_update_vertices, tet_mesh.cu:12-20
	warp_box(de.bbox, de.aabb, de.warped_bbox);
	box_of(mesh->h_original_vertices, mesh->n_vertices, orig_bbox); // ctor, tet_mesh.h:100-107
	warp_box(orig_bbox, de.aabb, de.orig_warped_bbox);
	auto dev_alloc = [](auto& buf, size_t count) { return buf.alloc(count) == hipSuccess ? NRS_OK : fail(NRS_ERR_HIP, "nrs_edit_create: hipMalloc failed"); };
	NRS_TRY(upload(e->d_orig, mesh->h_original_vertices, 3 * (size_t)mesh->n_vertices));
	NRS_TRY(upload(e->d_tets, mesh->h_tets, 4 * (size_t)mesh->n_tets));
	de.orig = e->d_orig.get();
	de.tets = e->d_tets.get();
	NRS_TRY(dev_alloc(e->d_verts, 3 * (size_t)mesh->n_vertices));
	NRS_TRY(dev_alloc(e->d_lut_off, n_cells + 1));
	if (hipMemcpy(e->d_verts.get(), mesh->h_vertices, 12 * (size_t)mesh->n_vertices, hipMemcpyHostToDevice) != hipSuccess)
		return fail(NRS_ERR_HIP, "nrs_edit_create: vertex upload failed");
	NRS_TRY(dev_alloc(e->d_planes, 32 * (size_t)mesh->n_tets));
	NRS_TRY(dev_alloc(e->d_mapback, 24 * (size_t)mesh->n_tets));
	de.mapback = e->d_mapback.get();
	de.verts = e->d_verts.get();
	de.lut_off = e->d_lut_off.get();
	de.planes = e->d_planes.get();
	const bool want_rot = mesh->h_local_rotations != nullptr || mesh->correct_direction != 0;
	if (want_rot) {
		NRS_TRY(dev_alloc(e->d_rot, 9 * (size_t)mesh->n_tets));
		de.rot = e->d_rot.get();
	}
	NRS_TRY(dev_alloc(e->d_orig_bitfield, NRS_BITFIELD_BYTES));
	uint8_t* d_orig_bits = e->d_orig_bitfield.get();
	de.orig_bitfield = d_orig_bits;
	de.copy = mesh->copy;
	de.apply_poisson = mesh->apply_poisson;
	de.residual_amplitude = mesh->residual_amplitude;
	if (mesh->apply_poisson) {
		NRS_TRY(upload(e->d_shs, mesh->h_boundary_shs, 27 * (size_t)mesh->n_vertices));
		NRS_TRY(upload(e->d_out_density, mesh->h_boundary_outside_density, (size_t)mesh->n_vertices));
		NRS_TRY(upload(e->d_res_density, mesh->h_boundary_residual_density, (size_t)mesh->n_vertices));
		de.shs = e->d_shs.get(); de.out_density = e->d_out_density.get(); de.res_density = e->d_res_density.get();
	}
	// touched cells of the CANONICAL mesh (build_original_tet_grid, tet_mesh.cu:76): handed over, or built here
	if (mesh->h_original_bitfield) {
		if (hipMemcpy(d_orig_bits, mesh->h_original_bitfield, NRS_BITFIELD_BYTES, hipMemcpyHostToDevice) != hipSuccess)
			return fail(NRS_ERR_HIP, "nrs_edit_create: bitfield upload failed");
	} else {
		NRS_TRY(build_lut_on_device(e, de.orig, d_orig_bits, nullptr));
	}
	if (host_lut) {
		hipError_t he = hipMemcpy(e->d_lut_off.get(), mesh->h_lut_offsets, (n_cells + 1) * 4, hipMemcpyHostToDevice);
		e->d_lut_idx.reset(); // (a canonical-mesh build above may have left its list here)
		e->d_big_cells.reset(); // re-sized together with the list on the next device build
		if (he == hipSuccess) he = e->d_lut_idx.alloc(n_idx);
		if (he == hipSuccess && n_idx) he = hipMemcpy(e->d_lut_idx.get(), mesh->h_lut_idx, (size_t)n_idx * 4, hipMemcpyHostToDevice);
		if (he != hipSuccess) return fail_hip(he, "nrs_edit_create: LUT upload");
		e->lut_idx_cap = n_idx;
		e->lut_n_idx = n_idx;
		de.lut_idx = e->d_lut_idx.get();
		NRS_LAUNCH(launch_tet_planes(e->n_tets, e->d_verts.get(), de.tets, e->d_planes.get(), nullptr));
		if (hipDeviceSynchronize() != hipSuccess) return fail(NRS_ERR_HIP, "nrs_edit_create: tet_planes_kernel failed");
		NRS_TRY(build_fine_lut(e, nullptr)); // (the fine look-up table of the LUT that was handed over)
		if (mesh->h_local_rotations) {
			he = hipMemcpy(e->d_rot.get(), mesh->h_local_rotations, 36 * (size_t)mesh->n_tets, hipMemcpyHostToDevice);
			if (he != hipSuccess) return fail_hip(he, "nrs_edit_create: rotation upload");
		} else if (want_rot) {
			NRS_LAUNCH(launch_local_rotations(e->n_tets, e->d_verts.get(), de.orig, de.tets, e->d_rot.get(), nullptr, nullptr));
			if (hipDeviceSynchronize() != hipSuccess) return fail(NRS_ERR_HIP, "nrs_edit_create: rotation kernel failed");
		}
	} else {
		NRS_TRY(rebuild_after_vertices(e, nullptr, true)); // LUT (+ rotations) of the deformed mesh, on the device; an operator at rest: with its fine table
		if (mesh->h_local_rotations && hipMemcpy(e->d_rot.get(), mesh->h_local_rotations, 36 * (size_t)mesh->n_tets, hipMemcpyHostToDevice) != hipSuccess)
			return fail(NRS_ERR_HIP, "nrs_edit_create: rotation upload failed");
	}
	// the map-back records, whole: the canonical vertices and the rotations as they stand now, wherever they came from (a move rewrites the rotation part)
	NRS_LAUNCH(launch_tet_mapback(e->n_tets, de.orig, de.tets, e->d_rot.get(), e->d_mapback.get(), nullptr));
	if (hipDeviceSynchronize() != hipSuccess) return fail(NRS_ERR_HIP, "nrs_edit_create: tet_mapback_kernel failed");
	*out = owner.release();
	return NRS_OK;
}
// AffineBoundingBox bookkeeping (affine_bounding_box.cuh:40-101) for the boxes the kernels test.  R column-major.
namespace {
struct HostAffineBox { float center[3], scale[3], rot[9]; };
void affine_finish(const HostAffineBox& b, AffineBox& out) {
	// u = rot * scale.x * e_x etc.;  min = -0.5 * rot * scale + center
	for (int i = 0; i < 3; ++i) {
		out.u[i] = b.rot[i] * b.scale[0];
		out.v[i] = b.rot[3 + i] * b.scale[1];
		out.w[i] = b.rot[6 + i] * b.scale[2];
		// Eigen's 3-term reduction order x0 + (x1 + x2) in every small product / dot (Redux.h complete unrolling; see nrs_vec.cuh)
		out.mn[i] = ((-0.5f * b.rot[i]) * b.scale[0] + ((-0.5f * b.rot[3 + i]) * b.scale[1] + (-0.5f * b.rot[6 + i]) * b.scale[2])) + b.center[i];
		out.center[i] = b.center[i];
	}
	out.uu = out.u[0] * out.u[0] + (out.u[1] * out.u[1] + out.u[2] * out.u[2]);
	out.vv = out.v[0] * out.v[0] + (out.v[1] * out.v[1] + out.v[2] * out.v[2]);
	out.ww = out.w[0] * out.w[0] + (out.w[1] * out.w[1] + out.w[2] * out.w[2]);
}
void affine_warp_box(HostAffineBox& b, const Box3& aabb) { // warp_box, :90-97
	for (int i = 0; i < 3; ++i) {
		const float diag = aabb.mx[i] - aabb.mn[i];
		b.center[i] = (b.center[i] - aabb.mn[i]) / diag;
		b.scale[i] = b.scale[i] / diag;
	}
}
} // namespace

int nrs_edit_create_affine(nrs_ctx* ctx, const nrs_model_desc* desc, const nrs_affine_duplication* op, nrs_edit** out) {
	if (!ctx || !desc || !op || !out) return fail(NRS_ERR_INVALID_ARG, "nrs_edit_create_affine: NULL argument");
	for (int i = 0; i < 3; ++i)
		if (!(op->scale[i] != 0.f) || !(op->selection_scale[i] > 0.f)) return fail(NRS_ERR_INVALID_ARG, "nrs_edit_create_affine: zero scale / empty selection box");
	nrs_edit* e = new (std::nothrow) nrs_edit();
	if (!e) return fail(NRS_ERR_STATE, "out of host memory");
	e->ctx = ctx;
	DeviceEdit& de = e->de;
	de.kind = kEditAffine;
	for (int k = 0; k < 3; ++k) { de.aabb.mn[k] = desc->aabb_min[k]; de.aabb.mx[k] = desc->aabb_max[k]; }
	HostAffineBox sel, dst;
	memcpy(sel.center, op->selection_center, 12); memcpy(sel.scale, op->selection_scale, 12); memcpy(sel.rot, op->selection_rot, 36);
	// update_destination (affine_duplication.h:77-90): translate, scale_with_vector, rotate (rot_matrix = R * rot_matrix)
	dst = sel;
	for (int i = 0; i < 3; ++i) { dst.center[i] = dst.center[i] + op->translation[i]; dst.scale[i] = dst.scale[i] * op->scale[i]; }
	for (int c = 0; c < 3; ++c)
		for (int r = 0; r < 3; ++r)
			dst.rot[3 * c + r] = op->rotation[r] * sel.rot[3 * c] + (op->rotation[3 + r] * sel.rot[3 * c + 1] + op->rotation[6 + r] * sel.rot[3 * c + 2]);
	affine_warp_box(dst, de.aabb);
	affine_warp_box(sel, de.aabb);
	affine_finish(dst, de.a_dst);
	affine_finish(sel, de.a_sel);
	for (int i = 0; i < 3; ++i) {
		de.a_translation[i] = op->translation[i] / (de.aabb.mx[i] - de.aabb.mn[i]); // m_warped_translation
		de.a_scale[i] = op->scale[i];
	}
	memcpy(de.a_rot, op->rotation, 36);
	de.a_hide_original = op->hide_original ? 1u : 0u;
	de.a_correct_dir = op->correct_dir ? 1u : 0u;
	*out = e;
	return NRS_OK;
}
void nrs_edit_destroy(nrs_edit* e) {
	delete e; // (its buffers go with it)
}

// ---- per-move updates --------------------------------------------------------------------------------------------
int nrs_edit_set_mvc(nrs_edit* e, const float* h_weights, uint32_t n_cage_vertices) {
	if (!e || !h_weights || n_cage_vertices == 0) return fail(NRS_ERR_INVALID_ARG, "nrs_edit_set_mvc: bad argument");
	if (e->de.kind != kEditCage) return fail(NRS_ERR_STATE, "nrs_edit_set_mvc: not a cage operator");
	HIP_TRY(hipSetDevice(e->ctx->device));
	e->d_mvc.reset(); e->d_cage.reset();
	e->n_cv = 0;
	const size_t nw = (size_t)e->n_vertices * n_cage_vertices;
	HIP_TRY(e->d_mvc.alloc(nw));
	HIP_TRY(e->d_cage.alloc((size_t)n_cage_vertices * 3));
	HIP_TRY(hipMemcpy(e->d_mvc.get(), h_weights, nw * 4, hipMemcpyHostToDevice));
	e->n_cv = n_cage_vertices;
	return NRS_OK;
}
int nrs_edit_update_cage(nrs_edit* e, void* stream, const float* h_cage_vertices, uint32_t n_cage_vertices) {
	if (!e || !h_cage_vertices) return fail(NRS_ERR_INVALID_ARG, "nrs_edit_update_cage: NULL argument");
	if (!e->d_mvc.get()) return fail(NRS_ERR_STATE, "nrs_edit_update_cage: MVC weights not set (nrs_edit_set_mvc)");
	if (n_cage_vertices != e->n_cv) return fail(NRS_ERR_INVALID_ARG, "nrs_edit_update_cage: cage vertex count differs from the MVC weights'");
	HIP_TRY(hipSetDevice(e->ctx->device));
	hipStream_t s = (hipStream_t)stream;
	HIP_TRY(hipMemcpyAsync(e->d_cage.get(), h_cage_vertices, (size_t)n_cage_vertices * 12, hipMemcpyHostToDevice, s));
	NRS_LAUNCH(launch_mvc_apply(e->n_vertices, e->n_cv, e->d_mvc.get(), e->d_cage.get(), e->d_verts.get(), s));
	return rebuild_after_vertices(e, s);
}
// GrowingSelection::interpolate_poisson_boundary (growing_selection.cu:2350-2395): the link between nrs_poisson_boundary (per CAGE vertex) and the
// render kernel's membrane path (per TET vertex).  The per-cage-vertex factors are prepared here with the host libm's expf (the reference does this
// on the host: std::exp(float)); the V_tet x V_cage weighted sums run on the device in the reference's order.
int nrs_edit_poisson_interpolate(nrs_edit* e, void* stream, const float* h_gamma, uint32_t n_cage_vertices, const float* h_inside_density, const float* h_outside_density,
                                 const float* h_inside_shs, const float* h_outside_shs, float residual_amplitude) {
	if (!e || !h_inside_density || !h_outside_density || !h_inside_shs || !h_outside_shs || n_cage_vertices == 0) return fail(NRS_ERR_INVALID_ARG, "nrs_edit_poisson_interpolate: bad argument");
	if (e->de.kind != kEditCage) return fail(NRS_ERR_STATE, "nrs_edit_poisson_interpolate: not a cage operator");
	if (!h_gamma && (!e->d_mvc.get() || e->n_cv != n_cage_vertices))
		return fail(NRS_ERR_STATE, "nrs_edit_poisson_interpolate: no gamma coordinates given and the operator holds no MVC weights for this cage (nrs_edit_set_mvc)");
	HIP_TRY(hipSetDevice(e->ctx->device));
	hipStream_t s = (hipStream_t)stream;
	const float min_step = 1.73205080757f / 1024; // MIN_CONE_STEPSIZE(), common_nerf.h:31
	std::vector<float> per_cage((size_t)n_cage_vertices * 30);
	for (uint32_t j = 0; j < n_cage_vertices; ++j) {
		const float alpha_out = 1 - expf(-h_outside_density[j] * min_step), alpha_in = 1 - expf(-h_inside_density[j] * min_step);
		const float w_outside = 1.f, w_inside = std::min(alpha_in / alpha_out, 1.f);
		float* c = per_cage.data() + 30 * (size_t)j;
		c[0] = alpha_out;
		c[1] = h_outside_density[j];
		c[2] = h_outside_density[j] - h_inside_density[j];
		for (int k = 0; k < 27; ++k) c[3 + k] = w_outside * h_outside_shs[27 * (size_t)j + k] - w_inside * h_inside_shs[27 * (size_t)j + k];
	}
	DeviceBuffer<float> d_per_cage, d_gamma; // staging
	HIP_TRY(d_per_cage.alloc(per_cage.size()));
	if (hipMemcpyAsync(d_per_cage.get(), per_cage.data(), per_cage.size() * 4, hipMemcpyHostToDevice, s) != hipSuccess) return fail(NRS_ERR_HIP, "nrs_edit_poisson_interpolate: upload");
	if (h_gamma) {
		if (d_gamma.alloc((size_t)e->n_vertices * n_cage_vertices) != hipSuccess ||
		    hipMemcpyAsync(d_gamma.get(), h_gamma, (size_t)e->n_vertices * n_cage_vertices * 4, hipMemcpyHostToDevice, s) != hipSuccess)
			return fail(NRS_ERR_HIP, "nrs_edit_poisson_interpolate: upload of the gamma coordinates");
	}
	if (!e->de.shs) { // the operator was created without membrane arrays: they are the operator's from now on
		if (e->d_shs.alloc(27 * (size_t)e->n_vertices) != hipSuccess || e->d_out_density.alloc(e->n_vertices) != hipSuccess || e->d_res_density.alloc(e->n_vertices) != hipSuccess)
			return fail(NRS_ERR_HIP, "nrs_edit_poisson_interpolate: device allocation");
		e->de.shs = e->d_shs.get(); e->de.out_density = e->d_out_density.get(); e->de.res_density = e->d_res_density.get();
	}
	NRS_LAUNCH(launch_poisson_interpolate(e->n_vertices, n_cage_vertices, h_gamma ? d_gamma.get() : e->d_mvc.get(), d_per_cage.get(), e->d_shs.get(), e->d_out_density.get(),
	                                      e->d_res_density.get(), s));
	if (hipStreamSynchronize(s) != hipSuccess) return fail(NRS_ERR_HIP, "nrs_edit_poisson_interpolate: synchronise"); // the staging buffers are freed on return
	e->de.apply_poisson = 1u;
	e->de.residual_amplitude = residual_amplitude;
	return NRS_OK;
}
// the per-tet-vertex membrane terms an operator holds ([V*27], [V], [V]); any pointer may be NULL
int nrs_edit_download_poisson(nrs_edit* e, float* h_boundary_shs, float* h_outside_density, float* h_residual_density) {
	if (!e) return fail(NRS_ERR_INVALID_ARG, "nrs_edit_download_poisson: NULL argument");
	if (!e->de.shs) return fail(NRS_ERR_STATE, "nrs_edit_download_poisson: the operator holds no membrane terms");
	HIP_TRY(hipSetDevice(e->ctx->device));
	if (h_boundary_shs) HIP_TRY(hipMemcpy(h_boundary_shs, e->de.shs, 27 * (size_t)e->n_vertices * 4, hipMemcpyDeviceToHost));
	if (h_outside_density) HIP_TRY(hipMemcpy(h_outside_density, e->de.out_density, (size_t)e->n_vertices * 4, hipMemcpyDeviceToHost));
	if (h_residual_density) HIP_TRY(hipMemcpy(h_residual_density, e->de.res_density, (size_t)e->n_vertices * 4, hipMemcpyDeviceToHost));
	return NRS_OK;
}
int nrs_edit_update_vertices(nrs_edit* e, void* stream, const float* h_vertices, uint32_t n_vertices) {
	if (!e || !h_vertices) return fail(NRS_ERR_INVALID_ARG, "nrs_edit_update_vertices: NULL argument");
	if (e->de.kind != kEditCage) return fail(NRS_ERR_STATE, "nrs_edit_update_vertices: not a cage operator");
	if (n_vertices != e->n_vertices) return fail(NRS_ERR_INVALID_ARG, "nrs_edit_update_vertices: vertex count differs from the mesh's");
	HIP_TRY(hipSetDevice(e->ctx->device));
	hipStream_t s = (hipStream_t)stream;
	HIP_TRY(hipMemcpyAsync(e->d_verts.get(), h_vertices, (size_t)n_vertices * 12, hipMemcpyHostToDevice, s));
	return rebuild_after_vertices(e, s);
}
int nrs_edit_lut_size(const nrs_edit* e, uint32_t* n_idx, uint32_t* max_per_cell) {
	if (!e) return fail(NRS_ERR_INVALID_ARG, "nrs_edit_lut_size: NULL argument");
	if (n_idx) *n_idx = e->lut_n_idx;
	if (max_per_cell) *max_per_cell = e->lut_max_per_cell;
	return NRS_OK;
}
int nrs_edit_download(nrs_edit* e, float* h_vertices, uint32_t* h_lut_offsets, uint32_t* h_lut_idx, float* h_rotations, uint8_t* h_original_bitfield,
                      float* h_bbox6) {
	if (!e) return fail(NRS_ERR_INVALID_ARG, "nrs_edit_download: NULL argument");
	if (e->de.kind != kEditCage) return fail(NRS_ERR_STATE, "nrs_edit_download: not a cage operator");
	HIP_TRY(hipSetDevice(e->ctx->device));
	if (h_vertices) HIP_TRY(hipMemcpy(h_vertices, e->d_verts.get(), (size_t)e->n_vertices * 12, hipMemcpyDeviceToHost));
	if (h_lut_offsets) HIP_TRY(hipMemcpy(h_lut_offsets, e->d_lut_off.get(), ((size_t)kGridVol * kCascades + 1) * 4, hipMemcpyDeviceToHost));
	if (h_lut_idx && e->lut_n_idx) HIP_TRY(hipMemcpy(h_lut_idx, e->d_lut_idx.get(), (size_t)e->lut_n_idx * 4, hipMemcpyDeviceToHost));
	if (h_rotations) {
		if (!e->d_rot.get()) return fail(NRS_ERR_STATE, "nrs_edit_download: the edit has no local rotations");
		HIP_TRY(hipMemcpy(h_rotations, e->d_rot.get(), (size_t)e->n_tets * 36, hipMemcpyDeviceToHost));
	}
	if (h_original_bitfield) HIP_TRY(hipMemcpy(h_original_bitfield, e->de.orig_bitfield, NRS_BITFIELD_BYTES, hipMemcpyDeviceToHost));
	if (h_bbox6) { memcpy(h_bbox6, e->de.bbox.mn, 12); memcpy(h_bbox6 + 3, e->de.bbox.mx, 12); }
	return NRS_OK;
}
int nrs_edit_map_rays(nrs_edit* e, void* stream, uint32_t n, float* d_coords, uint8_t* d_empty_mask) {
	if (!e || !d_coords || !d_empty_mask) return fail(NRS_ERR_INVALID_ARG, "nrs_edit_map_rays: NULL argument");
	HIP_TRY(hipSetDevice(e->ctx->device));
	NRS_LAUNCH(launch_map_rays(e->de, n, d_coords, NRS_NETWORK_INPUT_FLOATS, 1, d_empty_mask, stream));
	return NRS_OK;
}
int nrs_edit_map_positions(nrs_edit* e, void* stream, uint32_t n, float* d_pos, uint32_t ld, uint8_t* d_empty_mask) {
	if (!e || !d_pos || !d_empty_mask) return fail(NRS_ERR_INVALID_ARG, "nrs_edit_map_positions: NULL argument");
	if (ld < 3) return fail(NRS_ERR_INVALID_ARG, "nrs_edit_map_positions: ld < 3");
	HIP_TRY(hipSetDevice(e->ctx->device));
	NRS_LAUNCH(launch_map_rays(e->de, n, d_pos, ld, 0, d_empty_mask, stream));
	return NRS_OK;
}

} // extern "C"
