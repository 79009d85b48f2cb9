// nrs_api_model.cpp -- the model: create / destroy, parameters, both cell-record caches, numerics, light direction, occupancy set / get / refresh.
#include "nrs_host.h"
#include "nrs_tables.h"
#include "nrs_occupancy.h"
#include "nrs_optimizer.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <new>

using namespace nrs;

// Both flavours of the marching accelerator from m->d_bitfield (launch_occ_accel: bounds, box and look-ahead masks are built on the device);
// the host reads back the 2 x 12 floats a launch carries in its kernel arguments, and synchronises the stream for that.
static int refresh_accel(nrs_model* m, void* stream) {
	hipStream_t s = (hipStream_t)stream;
	float* d_out = reinterpret_cast<float*>(m->d_accel_masks.get() + 2 * kCoarseWords);
	NRS_LAUNCH(launch_occ_accel(m->dm.bitfield, m->d_accel_masks.get(), d_out, m->d_accel_masks.get() + 2 * kCoarseWords + 24, stream));
	float h[24];
	HIP_TRY(hipMemcpyAsync(h, d_out, sizeof(h), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	OccAccel* acc[2] = {&m->accel_any, &m->accel_exact};
	for (int f = 0; f < 2; ++f)
		for (int k = 0; k < 3; ++k) {
			acc[f]->box.mn[k] = h[f * 12 + k];
			acc[f]->box.mx[k] = h[f * 12 + 3 + k];
			acc[f]->cell[k] = h[f * 12 + 6 + k];
			acc[f]->inv_cell[k] = h[f * 12 + 9 + k];
		}
	m->accel_any.mask = m->d_accel_masks.get();
	m->accel_exact.mask = m->d_accel_masks.get() + kCoarseWords;
	return NRS_OK;
}
// DeviceModel as one render / trace launch sees it: the marching accelerator that matches the launch's step parameters
DeviceModel nrs::model_for_launch(const nrs_model* m, const nrs_render_params& p) {
	DeviceModel dm = m->dm;
	dm.occ = (p.cone_angle_constant == 0.f && p.min_mip == 0) ? m->accel_exact : m->accel_any;
	return dm;
}
// bitfield + mips from m->d_density_grid, then the marching shortcut's bounds and masks (all on the device; synchronises for 96 bytes)
int nrs::model_refresh_bitfield(nrs_model* m, void* stream) {
	hipStream_t s = (hipStream_t)stream;
	HIP_TRY(hipMemsetAsync(m->d_bitfield.get(), 0, NRS_BITFIELD_BYTES, s));
	NRS_LAUNCH(launch_grid_to_bitfield(m->d_density_grid.get(), m->d_bitfield.get(), m->ctx->d_mean.get(), stream));
	NRS_TRY(refresh_accel(m, stream));
	m->have_bitfield = true;
	return NRS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
extern "C" {

static void update_light(nrs_model* m) { // m_nerf.light_dir.normalized() (testbed_nerf.cu:3135), then warp_direction in fp32 as the sample generators do (:649, :690)
	const float* l = m->light_dir;
	const float n = std::sqrt(l[0] * l[0] + l[1] * l[1] + l[2] * l[2]);
	for (int k = 0; k < 3; ++k) m->dm.light01[k] = (l[k] / n + 1.0f) * 0.5f;
}
int nrs_model_n_extra_dims(const nrs_model* m) { return m ? (int)m->n_extra_dims : 0; }
int nrs_model_set_light_dir(nrs_model* m, const float dir[3]) {
	if (!m || !dir) return fail(NRS_ERR_INVALID_ARG, "nrs_model_set_light_dir: NULL argument");
	const float n2 = dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2];
	if (!std::isfinite(n2) || !(n2 > 0.f)) return fail(NRS_ERR_INVALID_ARG, "nrs_model_set_light_dir: the direction must be finite and non-zero (it is normalised at use)");
	for (int k = 0; k < 3; ++k) m->light_dir[k] = dir[k];
	update_light(m);
	return NRS_OK;
}
static int model_create(nrs_ctx* ctx, const nrs_model_desc* desc, uint32_t n_extra_dims, nrs_model** out, const char* who) {
	if (!ctx || !desc || !out) return fail(NRS_ERR_INVALID_ARG, std::string(who) + ": NULL argument");
	if (n_extra_dims != 0u && n_extra_dims != 3u) return fail(NRS_ERR_UNSUPPORTED, "nrs_model_create_ex: n_extra_dims must be 0 or 3 (light directions, dataset.has_light_dirs)");
	if (desc_supported(*desc))
		if (const char* why = extra_dims_refusal(*desc, n_extra_dims)) return fail(NRS_ERR_UNSUPPORTED, std::string("nrs_model_create_ex: ") + why);
	if (!desc_supported(*desc)) return fail(NRS_ERR_UNSUPPORTED, "model description outside configs/nerf/base.json's family (hash grid 16 x 2, 64-wide density network of 0..1 hidden layers, rgb network of 0..3 hidden layers or none)");
	for (int k = 0; k < 3; ++k)
		if (!(desc->aabb_max[k] > desc->aabb_min[k])) return fail(NRS_ERR_INVALID_ARG, std::string(who) + ": empty aabb");
	HIP_TRY(hipSetDevice(ctx->device));
	nrs_model* m = new (std::nothrow) nrs_model();
	if (!m) return fail(NRS_ERR_STATE, "out of host memory");
	m->ctx = ctx;
	m->desc = *desc;
	m->total_entries = make_levels(*desc, m->dm.levels);
	for (int k = 0; k < 3; ++k) { m->dm.aabb.mn[k] = desc->aabb_min[k]; m->dm.aabb.mx[k] = desc->aabb_max[k]; }
	m->dm.diag_pow2 = 1;
	for (int k = 0; k < 3; ++k) {
		const float diag = desc->aabb_max[k] - desc->aabb_min[k];
		int e = 0;
		if (std::frexp(diag, &e) != 0.5f) m->dm.diag_pow2 = 0;
		m->dm.inv_diag[k] = 1.0f / diag;
	}
	m->dm.rgb_deep = desc->sh_degree != 0 && desc->rgb_hidden_layers == 3 ? 1u : 0u;
	m->dm.no_dir = desc->sh_degree == 0 ? 1u : 0u;
	m->n_extra_dims = m->dm.n_extra_dims = n_extra_dims;
	update_light(m);
	m->dm.rgb_activation = desc->rgb_activation;
	m->dm.density_activation = desc->density_activation;
	hipError_t he = m->d_grid.alloc(m->total_entries);
	if (he == hipSuccess) he = m->d_wfrag.alloc(kWfragDeviceBytes / 2);
	if (he == hipSuccess) he = m->d_bitfield.alloc(NRS_BITFIELD_BYTES);
	if (he == hipSuccess) he = m->d_accel_masks.alloc(2 * kCoarseWords + 64); // + 24 floats of OccAccel numbers + 12 words of scratch (refresh_accel)
	if (he == hipSuccess) he = hipMemset(m->d_accel_masks.get(), 0, 2 * kCoarseWords * 4);
	if (he == hipSuccess) he = m->d_density_grid.alloc((size_t)kGridVol * kCascades);
	if (he == hipSuccess) he = hipMemset(m->d_density_grid.get(), 0, (size_t)kGridVol * kCascades * 4);
	if (he != hipSuccess) {
		nrs_model_destroy(m);
		return fail_hip(he, n_extra_dims ? "nrs_model_create_ex: device allocation" : "nrs_model_create: device allocation");
	}
	m->dm.grid = m->d_grid.get();
	m->dm.wfrag = m->d_wfrag.get();
	m->dm.bitfield = m->d_bitfield.get();
	// The cell-record cache is OPT-IN since round 6 (a 24 MB model does not reserve gigabytes unasked): nrs_model_set_cell_cache(model, budget), or NRS_CELL_CACHE_GB in
	// the environment for a host that cannot be changed -- never more than a quarter of the free HBM.
	if (const char* e = getenv("NRS_CELL_CACHE_GB")) {
		size_t budget = (size_t)(atof(e) * 1073741824.0), free_b = 0, total_b = 0;
		if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = std::min(budget, free_b / 4);
		if (nrs_model_set_cell_cache(m, budget) != NRS_OK) (void)nrs_model_set_cell_cache(m, 0); // an optimisation: render without it
	}
	*out = m;
	return NRS_OK;
}
int nrs_model_create(nrs_ctx* ctx, const nrs_model_desc* desc, nrs_model** out) { return model_create(ctx, desc, 0u, out, "nrs_model_create"); }
int nrs_model_create_ex(nrs_ctx* ctx, const nrs_model_desc* desc, uint32_t n_extra_dims, nrs_model** out) { return model_create(ctx, desc, n_extra_dims, out, "nrs_model_create_ex"); }
void nrs_model_destroy(nrs_model* m) {
	delete m; // (its buffers go with it)
}
// Cell-record cache: plan (how many levels fit the budget), allocate, build.  Levels are cached from the coarsest up, an
// even number of them (the kernels evaluate levels in pairs), and their records share one allocation.
static uint32_t plan_cell_cache(const LevelParams* lv, size_t budget, LevelParams* out, size_t* bytes) {
	uint32_t n = 0;
	uint64_t records = 0, fit = 0;
	for (uint32_t l = 0; l < kLevels; ++l) {
		const uint64_t cells = (uint64_t)lv[l].resolution * lv[l].resolution * lv[l].resolution;
		if ((records + cells) * 32ull > budget || records + cells >= (1ull << 32) || lv[l].resolution >= 4096u) break; // (res < 4096: the gather's 24-bit index products, nrs_hashgrid.cuh mul24)
		records += cells;
		if (l & 1u) { n = l + 1; fit = records; }
	}
	uint64_t first = 0;
	for (uint32_t l = 0; l < kLevels; ++l) {
		out[l] = lv[l];
		out[l].cached = l < n ? 1u : 0u;
		out[l].rec_first = l < n ? (uint32_t)first : 0u;
		out[l].rec_res = l < n ? lv[l].resolution : 0u;
		out[l].rec_res2 = out[l].rec_res * out[l].rec_res;
		if (l < n) first += (uint64_t)lv[l].resolution * lv[l].resolution * lv[l].resolution;
	}
	*bytes = (size_t)fit * 32;
	return n;
}
static int rebuild_cell_cache(nrs_model* m, void* stream = nullptr, bool sync = true) {
	if (!m->have_params) return NRS_OK;
	if (m->cached_levels) NRS_LAUNCH(launch_cell_records(m->dm, m->cached_levels, m->d_records.get(), stream));
	for (uint32_t l = m->sparse_first; l < m->sparse_first + m->sparse_levels; ++l)
		NRS_LAUNCH(launch_brick_fill(m->dm, m->dm.levels[l], m->d_slots.get() + m->slot_first[l], m->slot_count[l], m->d_records2.get(), stream));
	if (sync) HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
	return NRS_OK;
}
static void drop_sparse_cell_cache(nrs_model* m) {
	m->d_bricks.reset(); m->d_slots.reset(); m->d_records2.reset();
	m->sparse_bytes = 0; m->sparse_first = m->sparse_levels = 0;
	for (uint32_t l = 0; l < kLevels; ++l)
		if (m->dm.levels[l].cached == 2u) { m->dm.levels[l].cached = 0; m->dm.levels[l].rec_first = m->dm.levels[l].rec_res = m->dm.levels[l].rec_res2 = m->dm.levels[l].tab_first = 0; }
	m->dm.records2 = nullptr; m->dm.bricks = nullptr;
}
// The brick tables, slot lists and (unfilled) records of nrs_model_set_sparse_cell_cache: for the levels after the dense ones, in pairs, while tables + records fit the
// budget.  The model holds no sparse records when this starts; after a failure the caller drops what it has left behind.  Its scratch buffers go when it returns.
static int mark_sparse_bricks(nrs_model* m, const uint8_t* h_mask_bitfield, size_t max_bytes) {
	const uint32_t first = m->cached_levels;
	DeviceBuffer<uint8_t> d_mask;
	DeviceBuffer<uint32_t> d_counter, d_tmp_table;
	hipError_t he = d_mask.alloc(NRS_BITFIELD_BYTES);
	if (he == hipSuccess) he = hipMemcpy(d_mask.get(), h_mask_bitfield, NRS_BITFIELD_BYTES, hipMemcpyHostToDevice);
	if (he == hipSuccess) he = d_counter.alloc(kLevels);
	if (he == hipSuccess) he = hipMemset(d_counter.get(), 0, 4 * kLevels);
	if (he != hipSuccess) { (void)hipGetLastError(); return fail(NRS_ERR_HIP, "nrs_model_set_sparse_cell_cache: out of device memory"); }
	// pass A: level by level, mark into a scratch table to COUNT the bricks the mask asks for (the set is deterministic, only the slot order is
	// not); accept level pairs while tables + slot lists + records fit the budget
	LevelParams lv[kLevels];
	uint32_t counts[kLevels] = {}, nbs[kLevels] = {};
	uint64_t used = 0, table_total = 0, bricks_total = 0;
	uint32_t n_ok = 0;
	for (uint32_t l = first; l + 1 < kLevels; l += 2) {
		uint64_t pair_bytes = 0, pair_tables = 0, pair_bricks = 0;
		bool ok = true;
		for (uint32_t k = l; k < l + 2 && ok; ++k) {
			const uint32_t nb = (m->dm.levels[k].resolution + kBrick - 1) / kBrick;
			const uint64_t entries = (uint64_t)nb * nb * nb;
			if (entries * 4ull > max_bytes - std::min<uint64_t>(max_bytes, used + pair_bytes) || table_total + pair_tables + entries >= (1ull << 32)) { ok = false; break; }
			if (d_tmp_table.alloc(entries) != hipSuccess || hipMemset(d_tmp_table.get(), 0, entries * 4ull) != hipSuccess) { (void)hipGetLastError(); ok = false; break; }
			lv[k] = m->dm.levels[k];
			lv[k].rec_res = nb; lv[k].rec_res2 = nb * nb; lv[k].tab_first = 0; lv[k].rec_first = 0;
			NRS_LAUNCH(launch_brick_mark(m->dm, lv[k], d_mask.get(), d_tmp_table.get(), d_counter.get() + k, nullptr, 0, nullptr));
			if (hipMemcpy(&counts[k], d_counter.get() + k, 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(NRS_ERR_HIP, "nrs_model_set_sparse_cell_cache: read-back");
			d_tmp_table.reset();
			nbs[k] = nb;
			pair_tables += entries; pair_bricks += counts[k];
			pair_bytes += entries * 4ull + (uint64_t)counts[k] * ((uint64_t)kBrickCells * 32ull + 4ull);
			if (dev_knob("NRS_SPARSE_LOG"))
				fprintf(stderr, "[nrs sparse] level %u: res %u, %u^3 bricks (table %.1f MB), %u bricks marked = %.2f GB of records\n", k, m->dm.levels[k].resolution, nb, entries * 4e-6,
				        counts[k], counts[k] * 16384e-9);
		}
		if (!ok || used + pair_bytes > max_bytes || (bricks_total + pair_bricks) * kBrickCells >= (1ull << 32)) break;
		used += pair_bytes; table_total += pair_tables; bricks_total += pair_bricks;
		n_ok += 2;
	}
	if (!n_ok || !bricks_total) return NRS_OK;
	// pass B: the real tables, slot lists and records of the accepted levels
	he = m->d_bricks.alloc(table_total);
	if (he == hipSuccess) he = hipMemset(m->d_bricks.get(), 0, table_total * 4ull);
	if (he == hipSuccess) he = m->d_slots.alloc(bricks_total);
	if (he == hipSuccess) he = m->d_records2.alloc(bricks_total * kBrickCells * 2ull);
	if (he == hipSuccess) he = hipMemset(d_counter.get(), 0, 4 * kLevels);
	if (he != hipSuccess) { (void)hipGetLastError(); return fail(NRS_ERR_HIP, "nrs_model_set_sparse_cell_cache: out of device memory (records)"); }
	m->dm.records2 = m->d_records2.get(); m->dm.bricks = m->d_bricks.get();
	uint64_t tab = 0, slot0 = 0;
	for (uint32_t l = first; l < first + n_ok; ++l) {
		lv[l].tab_first = (uint32_t)tab;
		lv[l].rec_first = (uint32_t)(slot0 * kBrickCells);
		NRS_LAUNCH(launch_brick_mark(m->dm, lv[l], d_mask.get(), m->d_bricks.get() + tab, d_counter.get() + l, m->d_slots.get() + slot0, counts[l], nullptr));
		m->slot_first[l] = (uint32_t)slot0; m->slot_count[l] = counts[l];
		lv[l].cached = 2u;
		m->dm.levels[l] = lv[l];
		tab += (uint64_t)nbs[l] * nbs[l] * nbs[l];
		slot0 += counts[l];
	}
	m->sparse_first = first; m->sparse_levels = n_ok;
	m->sparse_bytes = (size_t)used;
	return NRS_OK;
}
// Sparse brick records for the levels after the dense ones, in pairs, while tables + records fit the budget.
int nrs_model_set_sparse_cell_cache(nrs_model* m, const uint8_t* h_mask_bitfield, size_t max_bytes) {
	if (!m) return fail(NRS_ERR_INVALID_ARG, "nrs_model_set_sparse_cell_cache: NULL model");
	HIP_TRY(hipSetDevice(m->ctx->device));
	HIP_TRY(hipDeviceSynchronize()); // launches in flight may still read the old records
	drop_sparse_cell_cache(m);
	if (!h_mask_bitfield || !max_bytes) return NRS_OK;
	if (const int st = mark_sparse_bricks(m, h_mask_bitfield, max_bytes)) {
		drop_sparse_cell_cache(m);
		return st;
	}
	return m->sparse_levels ? rebuild_cell_cache(m) : NRS_OK;
}
size_t nrs_model_sparse_cell_cache_bytes(const nrs_model* m, uint32_t* first_level, uint32_t* n_levels) {
	if (!m) return 0;
	if (first_level) *first_level = m->sparse_first;
	if (n_levels) *n_levels = m->sparse_levels;
	return m->sparse_bytes;
}
int nrs_model_set_cell_cache(nrs_model* m, size_t max_bytes) {
	if (!m) return fail(NRS_ERR_INVALID_ARG, "nrs_model_set_cell_cache: NULL model");
	HIP_TRY(hipSetDevice(m->ctx->device));
	HIP_TRY(hipDeviceSynchronize()); // launches in flight may still read the old records
	drop_sparse_cell_cache(m); // they start where the dense levels end: set them again afterwards
	LevelParams lv[kLevels];
	size_t bytes = 0;
	const uint32_t n = plan_cell_cache(m->dm.levels, max_bytes, lv, &bytes);
	if (bytes != m->records_bytes) {
		m->d_records.reset();
		m->records_bytes = 0;
		m->cached_levels = 0;
		for (uint32_t l = 0; l < kLevels; ++l) { m->dm.levels[l].cached = 0; }
		m->dm.records = nullptr;
		if (bytes && m->d_records.alloc(bytes / sizeof(uint4)) != hipSuccess) {
			(void)hipGetLastError();
			return fail(NRS_ERR_HIP, "nrs_model_set_cell_cache: out of device memory for the cell records");
		}
		m->records_bytes = bytes;
	}
	m->cell_cache_budget = max_bytes;
	m->cached_levels = n;
	for (uint32_t l = 0; l < kLevels; ++l) m->dm.levels[l] = lv[l];
	m->dm.records = m->d_records.get();
	return rebuild_cell_cache(m);
}
size_t nrs_model_cell_cache_bytes(const nrs_model* m, uint32_t* n_levels) {
	if (!m) return 0;
	if (n_levels) *n_levels = m->cached_levels;
	return m->records_bytes;
}

// ---- shared with the optimiser (nrs_optimizer.h): the two halves of nrs_model_set_params_device ------------------------------------------------------------
} // extern "C"
void nrs::model_param_counts(const nrs_model* m, uint32_t* n_mlp, size_t* n_params) {
	const uint32_t k = n_mlp_weights(m->desc, m->n_extra_dims);
	if (n_mlp) *n_mlp = k;
	if (n_params) *n_params = (size_t)k + (size_t)m->total_entries * 2;
}
uint16_t* nrs::model_grid_fp16(nrs_model* m) { return (uint16_t*)m->d_grid.get(); }
int nrs::model_mlp_from_device(nrs_model* m, const uint16_t* d, void* stream) {
	if (!m->d_wfrag_src.get()) { // the fragment permutation as indices: run the host routine on the identity (index + 1; 0 stays "padding")
		static_assert(kDensityW + 64 * 48 + 2 * 64 * 64 + 16 * 64 < kFragNegate, "weight indices + 1 fit 15 bits");
		std::vector<uint16_t> ident(n_mlp_weights(m->desc, m->n_extra_dims)), canon(kCanonW), src(kWfragDeviceBytes / 2);
		for (size_t i = 0; i < ident.size(); ++i) ident[i] = (uint16_t)(i + 1);
		lower_weights(m->desc, ident.data(), canon.data(), kLowerIndices, m->n_extra_dims);
		make_weight_fragments(canon.data(), src.data(), kFragOne);
		DeviceBuffer<uint16_t> fresh;
		HIP_TRY(fresh.alloc(kWfragDeviceBytes / 2));
		const hipError_t up = hipMemcpy(fresh.get(), src.data(), kWfragDeviceBytes, hipMemcpyHostToDevice);
		if (up != hipSuccess) return fail_hip(up, "nrs_model_set_params_device: upload of the weight permutation");
		m->d_wfrag_src = std::move(fresh); // (never keep a permutation that was not uploaded: later calls would scramble the weights silently)
	}
	NRS_LAUNCH(launch_weight_fragments(d, m->d_wfrag_src.get(), (uint16_t*)m->d_wfrag.get(), kWfragDeviceBytes / 2, stream));
	return NRS_OK;
}
int nrs::model_grid_written(nrs_model* m, void* stream) {
	m->have_params = true;
	return rebuild_cell_cache(m, stream, false);
}
extern "C" {

int nrs_model_set_params(nrs_model* m, const void* h_params_fp16, size_t n_params) {
	if (!m || !h_params_fp16) return fail(NRS_ERR_INVALID_ARG, "nrs_model_set_params: NULL argument");
	const uint32_t n_mlp = n_mlp_weights(m->desc, m->n_extra_dims);
	const size_t expect = (size_t)n_mlp + (size_t)m->total_entries * 2;
	if (n_params != expect) {
		char buf[160];
		snprintf(buf, sizeof(buf), "nrs_model_set_params: got %zu params, the description implies %zu", n_params, expect);
		return fail(NRS_ERR_INVALID_ARG, buf);
	}
	HIP_TRY(hipSetDevice(m->ctx->device));
	const uint16_t* w = (const uint16_t*)h_params_fp16;
	std::vector<uint16_t> canon(kCanonW), frag(kWfragDeviceBytes / 2);
	lower_weights(m->desc, w, canon.data(), kLowerValues, m->n_extra_dims);
	make_weight_fragments(canon.data(), frag.data());
	HIP_TRY(hipMemcpy(m->d_wfrag.get(), frag.data(), kWfragDeviceBytes, hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(m->d_grid.get(), w + n_mlp, (size_t)m->total_entries * 4, hipMemcpyHostToDevice));
	m->have_params = true;
	return rebuild_cell_cache(m);
}
// NerfNetworkFull::set_params hands over DEVICE pointers into the trainer's parameter blob (nerf_network_full.h:316-349): the same for a caller
// whose parameters already live on the device (a viewer that trains while it renders, src/testbed.cu:2502).  Everything is enqueued on `stream` and
// nothing waits: the hash grid (24-27 MB) is copied device-to-device (~10 us), the 20 KB of MLP weights are re-arranged into MFMA fragments by a
// small kernel (the permutation is make_weight_fragments', uploaded once per model), the cell records -- if the caller keeps any -- are rebuilt
// behind them.  Renders enqueued on the same stream afterwards see the new parameters; the blob may be overwritten once the stream has passed
// this call.  Copy semantics: call it again after every optimiser step (the reference's renderer reads the blob in place; ours is a transformed copy).
int nrs_model_set_params_device(nrs_model* m, const void* d_params_fp16, size_t n_params, void* stream) {
	if (!m || !d_params_fp16) return fail(NRS_ERR_INVALID_ARG, "nrs_model_set_params_device: NULL argument");
	const uint32_t n_mlp = n_mlp_weights(m->desc, m->n_extra_dims);
	const size_t expect = (size_t)n_mlp + (size_t)m->total_entries * 2;
	if (n_params != expect) {
		char buf[160];
		snprintf(buf, sizeof(buf), "nrs_model_set_params_device: got %zu params, the description implies %zu", n_params, expect);
		return fail(NRS_ERR_INVALID_ARG, buf);
	}
	HIP_TRY(hipSetDevice(m->ctx->device));
	const uint16_t* d = (const uint16_t*)d_params_fp16;
	NRS_TRY(model_mlp_from_device(m, d, stream));
	HIP_TRY(hipMemcpyAsync(m->d_grid.get(), d + n_mlp, (size_t)m->total_entries * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
	return model_grid_written(m, stream);
}
int nrs_model_set_numerics(nrs_model* m, uint32_t grid_acc, uint32_t mlp_acc) {
	if (!m) return fail(NRS_ERR_INVALID_ARG, "nrs_model_set_numerics: NULL model");
	if (grid_acc > NRS_GRID_ACC_NETWORK || mlp_acc > NRS_MLP_ACC_FP16) return fail(NRS_ERR_INVALID_ARG, "nrs_model_set_numerics: unknown mode");
	m->dm.numerics = (grid_acc == NRS_GRID_ACC_NETWORK ? 1u : 0u) | (mlp_acc == NRS_MLP_ACC_FP16 ? 2u : 0u);
	return NRS_OK;
}
int nrs_model_set_density_bitfield(nrs_model* m, const uint8_t* h_bitfield, size_t n_bytes) {
	if (!m || !h_bitfield) return fail(NRS_ERR_INVALID_ARG, "nrs_model_set_density_bitfield: NULL argument");
	if (n_bytes != NRS_BITFIELD_BYTES) return fail(NRS_ERR_INVALID_ARG, "nrs_model_set_density_bitfield: expected 5*128^3/8 bytes");
	HIP_TRY(hipSetDevice(m->ctx->device));
	HIP_TRY(hipMemcpy(m->d_bitfield.get(), h_bitfield, n_bytes, hipMemcpyHostToDevice));
	NRS_TRY(refresh_accel(m, nullptr));
	m->have_bitfield = true;
	return NRS_OK;
}
int nrs_model_set_density_grid(nrs_model* m, const float* h_grid, size_t n_floats) {
	if (!m || !h_grid) return fail(NRS_ERR_INVALID_ARG, "nrs_model_set_density_grid: NULL argument");
	if (n_floats != (size_t)kGridVol * kCascades) return fail(NRS_ERR_INVALID_ARG, "nrs_model_set_density_grid: expected 5*128^3 floats");
	HIP_TRY(hipSetDevice(m->ctx->device));
	HIP_TRY(hipMemcpy(m->d_density_grid.get(), h_grid, n_floats * 4, hipMemcpyHostToDevice));
	return model_refresh_bitfield(m, nullptr);
}
int nrs_model_get_density_grid(nrs_model* m, float* h_out, size_t n_floats) {
	if (!m || !h_out || n_floats != (size_t)kGridVol * kCascades) return fail(NRS_ERR_INVALID_ARG, "nrs_model_get_density_grid: bad argument");
	HIP_TRY(hipSetDevice(m->ctx->device));
	HIP_TRY(hipMemcpy(h_out, m->d_density_grid.get(), n_floats * 4, hipMemcpyDeviceToHost));
	return NRS_OK;
}

// tcnn::pcg32 on the host: only seeding and the skip-ahead (the refresh's two draws, a training step's advance)
static const uint64_t kPcgMult = 0x5851f42d4c957f2dULL;
static uint64_t pcg_advance(uint64_t state, uint64_t inc, uint64_t delta) {
	uint64_t cur_mult = kPcgMult, cur_plus = inc, acc_mult = 1u, acc_plus = 0u;
	while (delta > 0) {
		if (delta & 1) { acc_mult *= cur_mult; acc_plus = acc_plus * cur_mult + cur_plus; }
		cur_plus = (cur_mult + 1) * cur_plus;
		cur_mult *= cur_mult;
		delta >>= 1;
	}
	return acc_mult * state + acc_plus;
}
void nrs_rng_advance(uint64_t* state, uint64_t inc, uint64_t delta) {
	if (state) *state = pcg_advance(*state, inc, delta);
}
void nrs_rng_seed(uint64_t seed, uint64_t* state_out, uint64_t* inc_out) {
	const uint64_t inc = (1u << 1u) | 1u; // initseq = 1
	uint64_t state = 0u;
	state = state * kPcgMult + inc;
	state += seed;
	state = state * kPcgMult + inc;
	if (state_out) *state_out = state;
	if (inc_out) *inc_out = inc;
}

int nrs_model_update_density_grid(nrs_model* m, nrs_edit* const* edits, int n_edits, nrs_grid_update* u, void* stream) {
	if (!m || !u) return fail(NRS_ERR_INVALID_ARG, "nrs_model_update_density_grid: NULL argument");
	if (!m->have_params) return fail(NRS_ERR_STATE, "nrs_model_update_density_grid: parameters not set (nrs_model_set_params)");
	if (u->max_cascade >= kCascades) return fail(NRS_ERR_INVALID_ARG, "nrs_model_update_density_grid: max_cascade must be < 5");
	if (n_edits < 0 || n_edits > nrs_ctx::kMaxEdits) return fail(NRS_ERR_INVALID_ARG, "nrs_model_update_density_grid: too many edit operators");
	if (n_edits > 0 && !edits) return fail(NRS_ERR_INVALID_ARG, "nrs_model_update_density_grid: edits is NULL");
	if ((uint64_t)u->n_uniform_samples + u->n_nonuniform_samples > 0x40000000ull)
		return fail(NRS_ERR_INVALID_ARG, "nrs_model_update_density_grid: more than 2^30 samples");
	nrs_ctx* ctx = m->ctx;
	HIP_TRY(hipSetDevice(ctx->device));
	hipStream_t s = (hipStream_t)stream;
	const size_t grid_bytes = (size_t)kGridVol * kCascades * 4;
	if (!m->d_density_tmp.get()) HIP_TRY(m->d_density_tmp.alloc((size_t)kGridVol * kCascades));
	DeviceEdit* d_refresh_edits = ctx->d_edits.get() + (size_t)nrs_ctx::kInFlight * nrs_ctx::kMaxEdits; // the refresh's own operator table
	if (n_edits > 0) {
		DeviceEdit host_edits[nrs_ctx::kMaxEdits];
		for (int i = 0; i < n_edits; ++i) {
			if (!edits[i]) return fail(NRS_ERR_INVALID_ARG, "nrs_model_update_density_grid: NULL edit operator");
			host_edits[i] = edits[i]->de;
		}
		HIP_TRY(hipMemcpyAsync(d_refresh_edits, host_edits, sizeof(DeviceEdit) * n_edits, hipMemcpyHostToDevice, s));
		HIP_TRY(hipStreamSynchronize(s)); // host_edits is a stack array
	}
	if (u->reset_grid) HIP_TRY(hipMemsetAsync(m->d_density_grid.get(), 0, grid_bytes, s));
	HIP_TRY(hipMemsetAsync(m->d_density_tmp.get(), 0, grid_bytes, s));
	const uint64_t rng_nonuniform = pcg_advance(u->rng_state, u->rng_inc, 1ull << 32); // m_rng.advance() between the two draws
	NRS_LAUNCH(launch_grid_update(m->dm, d_refresh_edits, n_edits, *u, rng_nonuniform, m->d_density_grid.get(), m->d_density_tmp.get(), ctx->n_cus, stream));
	u->rng_state = pcg_advance(u->rng_state, u->rng_inc, 2ull << 32);
	u->ema_step += 1;
	return model_refresh_bitfield(m, stream);
}
int nrs_model_get_march_accelerator(nrs_model* m, int which, float* h_box12, uint32_t* h_mask) {
	if (!m || !h_box12 || !h_mask || which < 0 || which > 1) return fail(NRS_ERR_INVALID_ARG, "nrs_model_get_march_accelerator: bad argument");
	if (!m->have_bitfield) return fail(NRS_ERR_STATE, "nrs_model_get_march_accelerator: occupancy not set (nrs_model_set_density_bitfield/_grid)");
	HIP_TRY(hipSetDevice(m->ctx->device));
	const OccAccel& a = which ? m->accel_exact : m->accel_any;
	for (int k = 0; k < 3; ++k) { h_box12[k] = a.box.mn[k]; h_box12[3 + k] = a.box.mx[k]; h_box12[6 + k] = a.cell[k]; h_box12[9 + k] = a.inv_cell[k]; }
	HIP_TRY(hipMemcpy(h_mask, a.mask, kCoarseWords * 4, hipMemcpyDeviceToHost));
	return NRS_OK;
}
int nrs_model_get_density_bitfield(nrs_model* m, uint8_t* h_out, size_t n_bytes) {
	if (!m || !h_out || n_bytes != NRS_BITFIELD_BYTES) return fail(NRS_ERR_INVALID_ARG, "nrs_model_get_density_bitfield: bad argument");
	HIP_TRY(hipSetDevice(m->ctx->device));
	HIP_TRY(hipMemcpy(h_out, m->d_bitfield.get(), n_bytes, hipMemcpyDeviceToHost));
	return NRS_OK;
}

} // extern "C"
