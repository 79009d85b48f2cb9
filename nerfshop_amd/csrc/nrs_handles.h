// nrs_handles.h -- the opaque structs of include/nrs.h (context, model, edit, selection, dataset, optimiser, environment map, exposure), the error helpers and the owner of a device allocation: what a host unit behind the C-ABI needs to
// work on a context or a model.  nrs_host.h adds the helpers that cross the borders of the older units; a unit that needs none of them (nrs_api_mesh.cpp, nrs_api_selection.cpp) includes
// this header alone.  Host-only C++17: no .hip / .cuh includes it.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <deque>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/nrs.h"
#include "nrs_internal.h"
#include "nrs_render.h"

namespace nrs {

// The thread-local message behind nrs_last_error() (nrs_api.cpp): both set it and return the status.
int fail(int code, const std::string& msg);
int fail_hip(hipError_t e, const char* what); // "<what>: <HIP's error string>", NRS_ERR_HIP

// a HIP runtime call: the message quotes the failing expression
#define HIP_TRY(call)                                           \
	do {                                                        \
		hipError_t e_ = (call);                                 \
		if (e_ != hipSuccess) return nrs::fail_hip(e_, #call);  \
	} while (0)
// a host function that has set the message itself (fail / fail_hip / one of these macros): hand its status on
#define NRS_TRY(call)                   \
	do {                                \
		int s_ = (call);                \
		if (s_ != NRS_OK) return s_;    \
	} while (0)
// a launch_* function of the device units: they report through launch_last_error() (nrs_launch.cpp)
#define NRS_LAUNCH(call)                                                  \
	do {                                                                  \
		int s_ = (call);                                                  \
		if (s_ != NRS_OK) return nrs::fail(s_, nrs::launch_last_error()); \
	} while (0)

// The one owner of a device allocation: `count` elements of T from hipMalloc, freed when the owner goes.  Move-only.
template <typename T>
class DeviceBuffer {
public:
	DeviceBuffer() = default;
	DeviceBuffer(DeviceBuffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
	DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
		if (this != &o) {
			reset();
			p_ = std::exchange(o.p_, nullptr);
			n_ = std::exchange(o.n_, 0);
		}
		return *this;
	}
	DeviceBuffer(const DeviceBuffer&) = delete;
	DeviceBuffer& operator=(const DeviceBuffer&) = delete;
	~DeviceBuffer() { reset(); }
	// frees what it holds, then allocates (never less than 16 bytes: an empty array still has an address); holds nothing after a failure
	hipError_t alloc(size_t count) {
		reset();
		const hipError_t e = hipMalloc((void**)&p_, std::max<size_t>(count * sizeof(T), 16));
		if (e != hipSuccess) p_ = nullptr;
		else n_ = count;
		return e;
	}
	void reset() {
		if (p_) (void)hipFree(p_);
		p_ = nullptr;
		n_ = 0;
	}
	T* get() const { return p_; }
	size_t count() const { return n_; }

private:
	T* p_ = nullptr;
	size_t n_ = 0;
};

// marching_cubes_gpu + compute_mesh_1ring on a lattice that is already on the device (nrs_api_mesh.cpp; the arguments have been checked); `fn` names the caller in messages
int mesh_from_lattice(int device, void* stream, const uint32_t res3d[3], const float aabb_min[3], const float aabb_max[3], float thresh, const float* d_density,
                      nrs_mesh** mesh_out, const char* fn);
// mean, bitfield, mips and the marching accelerator from m->d_density_grid (nrs_api_model.cpp; waits for `stream`): what follows every change of the density grid
int model_refresh_bitfield(nrs_model* m, void* stream);

} // namespace nrs

struct nrs_ctx {
	int lane_teams = 0; // nrs_ctx_set_lane_teams: 0 = automatic, 1 / 2 / 4 = lanes per ray for every render launch
	int handover = -1;  // nrs_ctx_set_ray_handover: -1 = default (on; NRS_STEAL=0 turns it off), 0 / 1
	unsigned long long last_handover = 0; // rays | hand-overs << 32 of the last launch that returned statistics
	unsigned long long render_dispatches = 0; // render-kernel dispatches enqueued through this context, and the schedule of the last one (nrs_ctx_render_launches; under launch_mutex)
	uint32_t last_schedule = 0;
	int device = 0;
	int n_cus = 0;
	size_t hbm_bytes = 0;
	char name[256] = {0};
	// per-launch scratch comes from small rings so that render calls issued back to back on DIFFERENT streams (double-buffered
	// frames) do not share a packet counter or an operator table: slot = launch number % kInFlight
	static constexpr int kInFlight = 8;
	nrs::DeviceBuffer<nrs::RenderCounters> d_counters;   // [kInFlight][2]: the render kernel of a slot zeroes the OTHER block for the slot's next launch (no memset between frames)
	uint8_t counter_parity[kInFlight] = {};   // block the slot's next launch uses; counters_clean: that block is known to be zero
	bool counters_clean[kInFlight] = {};
	nrs::DeviceBuffer<nrs::DeviceEdit> d_edits;          // [kInFlight + 1][kMaxEdits]; the last table belongs to the occupancy refresh
	nrs::DeviceBuffer<nrs_sample_view> d_views;     // [kInFlight][NRS_SPP_BATCH_MAX]: the view table of a slot's launch (nrs_render_nerf_spp_views)
	std::atomic<uint32_t> launch_serial{0};
	std::mutex launch_mutex; // slot acquisition .. launch enqueued: two threads rendering on one ctx must not share a slot's counter block / parity
	// A slot is reused every kInFlight launches, possibly from ANOTHER stream: the launch that used it last records slot_done, and a
	// launch on a different stream makes its stream wait on that event before it clears the counters / re-sends the operator table
	// (same-stream reuse is ordered by the stream itself).
	hipEvent_t slot_done[kInFlight] = {};
	hipStream_t slot_stream[kInFlight] = {};
	bool slot_used[kInFlight] = {};
	nrs::DeviceBuffer<float> d_mean;
	nrs::DeviceBuffer<unsigned long long> d_wave_log; // profiling only (NRS_DEBUG & 4)
	unsigned long long* h_feedback = nullptr; // pinned, device-visible: written by the last workgroup of a render launch
	unsigned long long* d_feedback = nullptr; // its device address
	std::vector<nrs::DeviceEdit> edits_shadow = std::vector<nrs::DeviceEdit>((size_t)kInFlight * 32); // what each slot of d_edits holds
	int shadow_n[kInFlight] = {-1, -1, -1, -1, -1, -1, -1, -1};
	static constexpr int kMaxEdits = 32;
};

// (the cell-record cache's measured optimum on 1080p lego is 10 GiB = levels 0..11 of base.json's table, 9.2 GB: 12 levels 8.80, 14 levels (64 GB) 8.64, 10 levels 8.52,
// none 8.05 Gsamples/s -- the budget a caller who opts in would pass: include/nrs.h MEMORY NOTE)

struct nrs_model {
	nrs_ctx* ctx = nullptr;
	nrs_model_desc desc{};
	uint32_t n_extra_dims = 0;      // 0, or 3: trained with light directions (nrs_model_create_ex)
	float light_dir[3] = {0.5f, 0.5f, 0.5f}; // m_nerf.light_dir as the caller set it (testbed.h:639); normalised at use -> dm.light01
	nrs::DeviceModel dm{};
	uint32_t total_entries = 0;
	nrs::DeviceBuffer<uint32_t> d_grid;
	nrs::DeviceBuffer<uint16_t> d_wfrag;
	nrs::DeviceBuffer<uint16_t> d_wfrag_src;     // make_weight_fragments as a permutation (source index + 1, 0 = padding), for nrs_model_set_params_device
	nrs::DeviceBuffer<uint8_t> d_bitfield;
	nrs::DeviceBuffer<uint32_t> d_accel_masks;   // 2 x kCoarseWords: accel_any.mask | accel_exact.mask
	nrs::OccAccel accel_any{}, accel_exact{}; // marching shortcuts for general step parameters / for cone_angle == 0 && min_mip == 0
	nrs::DeviceBuffer<float> d_density_grid;   // m_nerf.density_grid [5*128^3], kept for the occupancy refresh
	nrs::DeviceBuffer<uint32_t> d_density_tmp; // density_grid_tmp (float bits), allocated on first refresh
	bool have_params = false, have_bitfield = false;
	// cell records of the first `cached_levels` levels (nrs_model_set_cell_cache)
	nrs::DeviceBuffer<uint4> d_records;
	size_t records_bytes = 0, cell_cache_budget = 0;
	uint32_t cached_levels = 0;
	// sparse brick records of the levels after them (nrs_model_set_sparse_cell_cache)
	nrs::DeviceBuffer<uint32_t> d_bricks;   // brick tables of the sparse levels, concatenated
	nrs::DeviceBuffer<uint32_t> d_slots;    // brick number of every allocated brick, per level (slot_first[l] .. +slot_count[l])
	nrs::DeviceBuffer<uint4> d_records2;
	size_t sparse_bytes = 0;        // tables + slots + records
	uint32_t sparse_first = 0, sparse_levels = 0;
	uint32_t slot_first[nrs::kLevels] = {}, slot_count[nrs::kLevels] = {};
	// per-ray workspace of nrs_training_samples / nrs_ray_loss (nrs_api_train.cpp): grown on the first call of a size, reused afterwards
	nrs::DeviceBuffer<uint32_t> d_train_ws;
};

struct nrs_edit {
	nrs_ctx* ctx = nullptr;
	nrs::DeviceEdit de{};
	uint32_t n_vertices = 0, n_tets = 0;
	// what a cage move does not rewrite
	nrs::DeviceBuffer<float> d_orig;           // == de.orig
	nrs::DeviceBuffer<uint32_t> d_tets;        // == de.tets
	nrs::DeviceBuffer<uint8_t> d_orig_bitfield; // == de.orig_bitfield
	nrs::DeviceBuffer<float> d_shs, d_out_density, d_res_density; // == de.shs / out_density / res_density once the operator holds membrane terms
	// device-side authoring state (nrs_cage.hip): everything a cage move rewrites
	nrs::DeviceBuffer<float> d_verts;          // == de.verts
	nrs::DeviceBuffer<uint32_t> d_lut_off;     // == de.lut_off, [5*128^3 + 1]
	nrs::DeviceBuffer<uint32_t> d_lut_idx;     // == de.lut_idx
	size_t lut_idx_cap = 0;            // entries allocated
	nrs::DeviceBuffer<float> d_rot;            // == de.rot when rotations are on
	nrs::DeviceBuffer<float> d_planes;         // == de.planes, [T x 32] one 128-byte record per tet (tet_planes_kernel), follows the deformed vertices
	nrs::DeviceBuffer<float> d_mapback;        // == de.mapback, [T x 24] one 96-byte record per tet: canonical vertices (written once), rotation (follows the deformed vertices with d_rot)
	nrs::DeviceBuffer<uint32_t> d_counts;      // [5*128^3], all zero between builds
	nrs::DeviceBuffer<uint32_t> d_tile_sums;
	nrs::DeviceBuffer<unsigned long long> d_hit_masks; // per (tet, cascade): the count pass's first 128 cell / tet tests (two words per item), reused by the fill pass (nrs_cage.hip tet_mark_kernel)
	nrs::DeviceBuffer<uint32_t> d_scratch;     // [0..5] bbox (float bits), [6] total entries, [7] max tets per cell, [8] long-list counter
	nrs::DeviceBuffer<uint32_t> d_big_cells;   // worklist of cells with long tet lists (sized with d_lut_idx)
	nrs::DeviceBuffer<float> d_mvc;            // [V x n_cv] weights
	nrs::DeviceBuffer<float> d_cage;           // [n_cv x 3]
	uint32_t n_cv = 0;
	uint32_t lut_n_idx = 0, lut_max_per_cell = 0;
	// fine look-up table under the LUT (DeviceEdit::fine_*, nrs_cage.hip): rebuilt with the LUT
	nrs::DeviceBuffer<uint32_t> d_fine_off;    // [fine_cells_cap + 1]
	nrs::DeviceBuffer<uint32_t> d_fine_counts; // [fine_cells_cap]
	nrs::DeviceBuffer<uint32_t> d_fine_idx;
	nrs::DeviceBuffer<uint2> d_fine_head;      // == de.fine_head when the table has head words, [fine_cells_cap]; dropped and rebuilt with d_fine_idx
	nrs::DeviceBuffer<uint32_t> d_fine_tiles;  // [kFineScanTiles]
	nrs::DeviceBuffer<int32_t> d_fine_win;     // [kCascades * 6] window + [30] total entries
	size_t fine_cells_cap = 0, fine_idx_cap = 0;
	uint32_t fine_n_idx = 0;
	// A cage MOVE does not rebuild the fine table (0.3 ms of a 1.0 ms move at 6 k tets): it drops it -- the kernels scan the LUT's own lists, as before round 6 -- and
	// the second nrs_render_nerf after the last move builds it (a gizmo drag renders one frame per move and never pays; a cage at rest renders 2-3 % faster)
	bool fine_stale = false;
	uint32_t renders_since_move = 0;
};

// RegionGrowing + GrowingSelection's morphology state (region_growing.h, growing_selection.h): host-only until a device call names a context
struct nrs_selection {
	std::vector<float> grid;            // m_density_grid_host [5 * 128^3]
	uint32_t max_cascade = 0;
	std::vector<uint8_t> bits;          // m_selection_grid_bitfield [NRS_BITFIELD_BYTES]
	std::vector<uint32_t> cells;        // m_selection_cell_idx, in order, duplicates kept (m_selection_points follows from it)
	std::deque<uint32_t> queue;         // m_growing_queue
	uint32_t level = 0;                 // m_growing_level
	bool performed_closing = false;
	int dilation_type = NRS_SE_CUBE, dilation_radius = 2, erosion_type = NRS_SE_SPHERE, erosion_radius = 2; // correct_mm_operations.h:70
	int device = -1;                    // of the buffers below, once a device call has allocated them
	nrs::DeviceBuffer<uint32_t> d_work; // [3][kMorphLevelWords]: the growing level in Morton order | two levels of rows
	nrs::DeviceBuffer<float> d_lattice; // [128^3]
};

// Posed images on the device (nrs_api_dataset.cpp, nrs_dataset.hip)
struct nrs_dataset {
	nrs_ctx* ctx = nullptr;
	uint32_t n_images = 0, width = 0, height = 0;
	nrs::DeviceBuffer<uint64_t> d_images;  // [n_images][height][width] fp16 RGBA, linear, premultiplied (NerfDataset::images_data)
	nrs::DeviceBuffer<float> d_cameras;    // [n_images][kCameraWords]
	nrs::DeviceBuffer<uint8_t> d_staging;  // one image of host pixels on its way to the conversion kernel, allocated by the first such image
	std::vector<float> cameras;            // what d_cameras holds once cameras_dirty is cleared
	std::vector<uint8_t> image_set, camera_set;
	uint32_t n_images_set = 0, n_cameras_set = 0;
	bool cameras_dirty = false;
	// the training error map (include/nrs.h, "the training error map"): 64-bit fixed-point cells, and the CDFs of the last build with their own resolution
	nrs::DeviceBuffer<uint64_t> d_error_map;   // [n_images][map_res_y][map_res_x]
	uint32_t map_res_x = 0, map_res_y = 0;     // 0: no map yet
	nrs::DeviceBuffer<float> d_cdf_x_cond_y, d_cdf_y, d_cdf_img, d_pmf_img, d_img_total; // d_img_total: the pictures' unnormalised totals (construct_cdf_1d's cdf_img)
	uint32_t cdf_res_x = 0, cdf_res_y = 0;
	bool cdf_valid = false;
};

// The optimiser's state (nrs_api_optimizer.cpp, nrs_optimizer.hip): every array in the blob's order, n elements.
struct nrs_optimizer {
	nrs_ctx* ctx = nullptr;
	nrs_model* model = nullptr;         // bound: the fp16 of the hash table is the model's resident table, d_fp16 holds the MLP weights only
	nrs_adam_params p{};
	uint32_t n = 0, n_matrix = 0;
	uint32_t split = 0;                 // elements of d_fp16: n when unbound, the number of MLP weights when bound
	nrs::DeviceBuffer<float> d_master, d_m, d_v, d_ema;
	nrs::DeviceBuffer<uint32_t> d_steps;
	nrs::DeviceBuffer<uint16_t> d_fp16;
	nrs::DeviceBuffer<float> d_table;   // [t_sat + 1]: bias(t) at index t
	uint32_t t_sat = 0;
	uint32_t step_count = 0;
	uint32_t variant = 0;               // NRS_OPTIMIZER_VARIANT at creation (measurements: nrs_optimizer.h)
	bool have_weights = false;
};

// The trainable environment map (nrs_api_envmap.cpp, nrs_envmap.hip).  The texels are the master weights of its own unbound optimiser: live = NRS_OPT_MASTER, EMA = NRS_OPT_EMA.
struct nrs_envmap {
	nrs_ctx* ctx = nullptr;
	uint32_t res_x = 0, res_y = 0;
	uint32_t n = 0;                              // 4 * res_x * res_y
	nrs_optimizer* opt = nullptr;                // n parameters, n_matrix = 0; owned
	nrs::DeviceBuffer<float> d_grad;             // [n]: zero between steps (the step clears what it reads)
	nrs::DeviceBuffer<unsigned long long> d_cells; // [n]: int64 fixed point, 2^-32 per unit; zero between steps
};

// Per-image exposure (nrs_api_exposure.cpp, nrs_exposure.hip): n = 3 * n_images elements per array.
struct nrs_exposure {
	nrs_ctx* ctx = nullptr;
	uint32_t n_images = 0;
	nrs_exposure_params p{};
	nrs::DeviceBuffer<float> d_values, d_m, d_v;
	nrs::DeviceBuffer<unsigned long long> d_cells; // int64 fixed point, 2^-32 per unit; zero after a step
	uint32_t step_count = 0;                       // one for all images
	uint32_t rays_accumulated = 0;                 // since the last step or set: at most 2^21
};
