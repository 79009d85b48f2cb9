// nrs_internal.h -- PODs shared between the C++ host code (nrs_api.cpp, nrs_api_*.cpp; their own header: nrs_host.h) and the HIP kernels (nrs_render*.hip, nrs_network.hip, nrs_display.hip, nrs_tables.hip, nrs_occupancy.hip, nrs_cage.hip, nrs_mesh.hip, nrs_selection.hip).
// Nothing here is part of the public ABI (that is include/nrs.h).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "../../include/nrs.h"
#include "nrs_route.h"

#include <stdlib.h>
#include <hip/hip_vector_types.h> // uint2 (DeviceEdit::fine_head), for the translation units that include nothing of HIP themselves

namespace nrs {

// Measurement knobs (NRS_DEBUG, NRS_TEAM, NRS_RENDER_CFG, NRS_TAIL_*, NRS_RETEAM, NRS_STEAL, the logs ...) are read from the environment ONLY when NRS_DEV_KNOBS is
// set: a production process ignores them.  The two documented overrides -- NRS_CELL_CACHE_GB (nrs.h) and NRS_RCCL_LIB (the RCCL test double, announced
// on stderr) -- are not knobs of this kind.  tools/*.sh and the probes set NRS_DEV_KNOBS=1.
inline const char* dev_knob(const char* name) {
	static const bool on = []() { const char* e = getenv("NRS_DEV_KNOBS"); return e && e[0] && e[0] != '0'; }();
	return on ? getenv(name) : nullptr;
}

constexpr uint32_t kGrid = 128;                  // NERF_GRIDSIZE
constexpr uint32_t kCascades = 5;                // NERF_CASCADES
constexpr uint32_t kGridVol = kGrid * kGrid * kGrid;
constexpr uint32_t kLevels = 16;
constexpr uint32_t kCoarse = 32;                // blocks per axis of the occupancy look-ahead mask
constexpr uint32_t kCoarseWords = kCoarse * kCoarse * kCoarse / 32;
static_assert((kCoarse & (kCoarse - 1)) == 0, "the block walk's bounds test (cx | cy | cz) needs a power of two");
constexpr uint32_t kDensityW = 64 * 32 + 16 * 64;           // density MLP params (base.json:30-36)
constexpr uint32_t kRgbW = 64 * 32 + 64 * 64 + 16 * 64;     // rgb MLP params (base.json:52-58)
// The kernels evaluate ONE network shape: base.json's (density 32 -> 64 -> 16, rgb 32 -> 64 -> 64 -> 16), plus an optional third rgb hidden layer.  The
// other members of configs/nerf/'s family -- rgb network with 0 / 1 / 3 hidden layers, no rgb network at all -- are LOWERED onto it when their parameters
// arrive (lower_weights, nrs_api_lowering.cpp): matrices of 0 / +-1 that reproduce the smaller network's values exactly.  The canonical blob the MFMA fragments are
// cut from: [Wd1 64x32 | Wd2 16x64 | Wr1 64x32 | Wr2 64x64 | Wr3 16x64 | Wr2b 64x64 (third hidden layer, base_3layer.json)].
// A network trained with light directions (n_extra_dims = 3) appends Wr1x [64 x 16]: columns 32..47 of its [64 x 48] first rgb matrix (the warped light
// direction and the Identity encoding's padding ones); zeros for every other network.
constexpr uint32_t kCanonW = kDensityW + kRgbW + 64 * 64 + 64 * 16;

// One hash-grid level as the kernels consume it (staged in LDS, 48 B).
struct LevelParams {
	float    scale;       // exp2(l*log2(b))*Nmin - 1
	uint32_t resolution;  // ceil(scale) + 1
	uint32_t res2;        // resolution^2
	uint32_t offset;      // first entry of the level in the concatenated table (in entries = u32 words)
	uint32_t count;       // entries in the level
	uint32_t hashed;      // 1: spatial hash (count is a power of two), 0: dense x + y*res + z*res^2
	uint32_t mask;        // count - 1 when hashed
	uint32_t cached;      // 1: the level has dense cell records (DeviceModel::records, nrs_model_set_cell_cache); 2: sparse brick records
	                      //    (DeviceModel::records2 + bricks, nrs_model_set_sparse_cell_cache)
	uint32_t rec_first;   // record number of cell (0, 0, 0) [dense] / of the level's first brick [sparse]
	uint32_t rec_res;     // dense: cells per side with a record (= resolution: every cell a position in [0,1]^3 can fall into); sparse: bricks per side
	uint32_t rec_res2;    // rec_res^2
	uint32_t tab_first;   // sparse: first entry of the level's brick table in DeviceModel::bricks
};

// MFMA A-operand image of the five weight matrices: kNumFrags fragments of 64 lanes x 8 halfs (1 KiB each).
// Fragment order (see nrs_mlp.cuh): D1[mb][ks] (4), D2[ks] (4), R1[mb][ks] (4), R2[mb][ks] (8), R3[ks] (4).
// Then two CONSTANT 0 / 1 fragments Sel0 / Sel1 (round 4): MFMA(Sel0, lo, 0) + MFMA(Sel1, hi, .) turn a D tile that was packed to fp16 (lo = rows of registers
// 0..7, hi = 8..15) back into fp32 accumulator registers exactly -- the fp16-accumulator model (NRS_MLP_ACC_FP16) rounds the running sum after every k step,
// and the way back from packed halfs through the matrix core costs two MFMA issues (the pipe is 10 % busy) instead of sixteen VALU conversions.
// These 26 fragments are staged into LDS.  Behind them, in HBM only: Bwd[ks] (4), the A operands of dL/dfeatures = W1^T dL/dhidden (render mode Normals),
// R2b[mb][ks] (8), the third hidden layer of an rgb network that has one (DeviceModel::rgb_deep; base_3layer.json), and R1L[mb] (2), the third k block of
// rgb layer 0 of a network trained with light directions (DeviceModel::n_extra_dims; rows in R1's order, k = 8 g + e <-> input column 32 + k).
// Last, the transposed operands of the backward pass (nrs_network_backward.hip stages them and Bwd into its own LDS): TD2[mb] (2), T1[ks] (4), T2[mb][ks] (8), T3[mb] (2).
constexpr uint32_t kNumFrags = 26;
constexpr uint32_t kNumFragsDevice = 56;
constexpr uint32_t kFragBytes = 64 * 8 * 2;
constexpr uint32_t kWfragBytes = kNumFrags * kFragBytes; // 26 KiB: the LDS image
constexpr uint32_t kWfragDeviceBytes = kNumFragsDevice * kFragBytes;
// make_weight_fragments on the identity permutation (nrs_model_set_params_device): an entry is a weight index + 1 (< 0x8000), bit 15 = "negated",
// 0 = padding, or one of the two constants
constexpr uint16_t kFragOne = 0xffffu, kFragMinusOne = 0xfffeu, kFragNegate = 0x8000u;

struct Box3 { float mn[3]; float mx[3]; };

// row pitch of the multi-GPU tile index (nrs.h, nrs_render_params::tile_size): odd, so that t mod (a power-of-two number of ranks) walks diagonals
inline uint32_t tile_pitch(uint32_t width, uint32_t tile_size) { return ((width + tile_size - 1u) / tile_size) | 1u; }

// Result-preserving marching accelerator derived from the occupancy bitfield (launch_occ_accel, on the device):
//   box   world-space bounds of every occupied cell that can be consulted, slightly inflated (shortcut 1)
//   mask  kCoarse^3 bits over box: bit (z*kCoarse + y)*kCoarse + x set iff such a cell (inflated alike) overlaps that block (shortcut 2)
struct OccAccel {
	Box3 box;
	float cell[3], inv_cell[3];
	const uint32_t* mask; // device, kCoarseWords words (staged into LDS by the kernels)
};

struct DeviceModel {
	const uint32_t* grid;      // fp16x2 entries
	const uint16_t* wfrag;     // kWfragBytes
	const uint8_t*  bitfield;  // NRS_BITFIELD_BYTES
	const void*     records;   // cell records of the cached levels: 2 x uint4 = the cell's 8 corner entries, x fastest
	const void*     records2;  // sparse levels: records of the allocated bricks, 512 records (8 x 8 x 8 cells, x fastest) per brick
	const uint32_t* bricks;    // sparse levels: brick tables, entry = brick slot + 1, or 0 = no records here (hashed gathers instead)
	LevelParams     levels[kLevels];
	Box3            aabb;      // train aabb (m_aabb)
	float           inv_diag[3]; // 1 / (aabb.max - aabb.min), exact when diag_pow2
	uint32_t        diag_pow2; // every aabb extent is a power of two (always so for NGP scene boxes): x / d == x * (1/d) bit for bit
	OccAccel        occ;       // marching shortcuts (filled per launch, see model_for_launch in nrs_api_model.cpp)
	uint32_t        rgb_activation;
	uint32_t        density_activation;
	uint32_t        numerics;  // bit 0: nrs_grid_acc NETWORK, bit 1: nrs_mlp_acc FP16 (nrs_model_set_numerics); 0 = the default roundings
	uint32_t        rgb_deep;  // the rgb network has a third hidden layer (fragments R2b, read from wfrag in HBM): base_3layer.json
	uint32_t        no_dir;    // NerfNetworkNoDir (base_nodir.json): the direction rows of caller batches are not read
	uint32_t        n_extra_dims; // 0, or 3: the network was trained with light directions (fragments R1L, read from wfrag in HBM)
	float           light01[3];   // warp_direction(normalised nrs_model_set_light_dir) in fp32: what every sample gets that brings no light direction of its own
};

// AffineBoundingBox as the kernels test it (affine_bounding_box.cuh:83-88): u.(p - min) in [0, u.u) etc.
struct AffineBox { float mn[3]; float u[3]; float v[3]; float w[3]; float uu, vv, ww; float center[3]; };
enum EditKind : uint32_t { kEditCage = 0, kEditAffine = 1 };

struct DeviceEdit {
	uint32_t kind;             // EditKind
	// AffineDuplication (affine_duplication.h:92-106): warped destination / selection boxes, warped translation
	uint32_t a_hide_original, a_correct_dir, a_pad;
	AffineBox a_dst, a_sel;
	float a_translation[3], a_scale[3], a_rot[9];
	Box3 aabb;                 // scene aabb
	float inv_diag[3];         // 1 / (aabb.max - aabb.min)
	uint32_t diag_pow2;        // every extent a power of two: x / d == x * (1 / d) bit for bit (DeviceModel::diag_pow2)
	Box3 bbox;                 // deformed mesh, world units           (TetMesh::bbox)
	Box3 warped_bbox;          // bbox in warped [0,1] coordinates     (TetMesh::warped_bbox)
	Box3 orig_warped_bbox;     // canonical mesh, warped               (TetMesh::original_warped_bbox)
	const uint32_t* lut_off;
	const uint32_t* lut_idx;
	const uint32_t* tets;
	const float*    verts;
	const float*    orig;
	const float*    rot;           // nullable
	// Fine look-up table under the reference's 128^3 one (round 6; nrs_cage.hip fine_*_kernel; nullable): every LUT cell of a cascade's window is cut into 4 x 4 x 4 (or 2 x 2 x 2) fine
	// cells, and a fine cell's list is its LUT cell's list FILTERED IN ORDER -- the tets whose four face tests can pass for some position of the fine cell (a conservative
	// box-against-half-spaces test on the very floats the scan compares) -- so the first containing tet is the one the reference's scan finds, after fewer candidates.
	const uint32_t* fine_off;      // CSR offsets over the windows' fine cells, cascade after cascade
	const uint32_t* fine_idx;
	int32_t         fine_win[kCascades][8]; // per cascade: first fine cell x, y, z, first offset index | extent x, y, z in fine cells (0: no tet reaches this cascade),
	                                        // log2 of the fine cells per LUT cell and axis (0..2) or kFinePlain: this cascade keeps the LUT's own lists
	const float*    planes;        // [T x 32] one 128-byte record per tet: its 4 vertices, the 4 face normals exactly as same_side_tet forms them, the 4 sign bits of dotV4 (tet_planes_kernel)
	// Head word per fine cell (nullable; never set without fine_off): .x = the list's first index into fine_idx, .y = the list's first tet in the low kFineHeadTetBits bits,
	// the list's length above them -- one 8-byte load instead of fine_off[cell], fine_off[cell + 1] and fine_idx[j0] (fine_lists_kernel<true> writes it with fine_idx)
	const uint2*    fine_head;     // [fine cells]
	// [T x 24] one 96-byte map-back record per tet: orig[tets[t].x .. w] (12 floats, tet_mapback_kernel at creation), the tet's rotation columns (9 floats, local_rotations_kernel
	// on every move; zero without rotations), 3 floats of padding -- with the plane record's vertices all that tet_warp reads of the tet it found
	const float*    mapback;
	const uint8_t*  orig_bitfield;
	const float*    shs;           // nullable unless apply_poisson
	const float*    out_density;
	const float*    res_density;
	float           residual_amplitude;
	uint32_t        copy;
	uint32_t        apply_poisson;
	uint32_t        pad;
};

struct RenderCounters {    // zeroed before every launch
	unsigned long long n_samples;
	uint32_t next_packet;
	uint32_t n_rays_alive;
	uint32_t n_rays_hit;
	uint32_t blocks_done; // workgroups that have flushed their statistics (the last one reports to RenderArgs::feedback)
	unsigned long long phase_cycles[8]; // NRS_DEBUG & 4: per-phase wave cycles (profiling build of the kernel only)
	// NRS_DEBUG & 4: voxel-walk statistics. [0]/[1] fill: lane iterations / wave trips (= max over lanes per call);
	// [2]/[3] the same for the per-sample march; [4] sample rounds, [5] live lanes summed over rounds, [6] march calls with > 1 trip
	// [8] samples inside a cage's deformed box (they scan a LUT cell), [9] rounds with such a sample, [10] candidates tested (lane iterations of the scan),
	// [11] the scan's wave trips (max over the lanes of a round), [12] samples that found their tet
	unsigned long long walk[13];
};

struct RenderArgs {
	nrs_render_params p;
	const DeviceEdit* edits;   // device array, applied last-to-first
	int32_t  n_edits;
	uint32_t any_poisson;      // some edit has apply_poisson set
	uint32_t any_affine;       // some edit is an AffineDuplication
	uint32_t extra;            // a render mode other than Shade / Cost, show_accel or dof != 0: render_kernel's EXTRA instantiation
	uint32_t gate;             // cone stepping (aabb_scale > 1 scenes): the plain kernel's GATE instantiation (L2 phase gate on the four finest hashed levels)
	uint32_t n_packets;        // pixel packets owned by this call (8x8 pixels; 8x4 / 4x4 with lane teams of 2 / 4)
	uint32_t tiles_x;          // image width in tiles (tiled mode) or in packets (whole-image mode)
	uint32_t packets_per_tile_x;
	uint32_t pixels_owned;     // pixels this launch covers (for the feedback word)
	unsigned long long* feedback; // host-mapped: rays that found an occupied cell | pixels_owned << 32, written by the last workgroup
	uint32_t tail_every;       // hybrid launches: every tail_every-th packet row is a tail row (3)
	uint32_t reteam;           // hybrid launches: spread a wave's last rays over its idle lanes (render_kernel)
	uint32_t tail_target;      // hybrid launches: rays a wave collects per generation once it works on tail packets (24)
	uint32_t all_tail;         // hybrid launches: every packet is a 4x4 tail packet (packet_pixel<4>'s geometry, whole-image or tiles)
	uint32_t steal;            // hybrid launches: waves that run out of work take half the rays of a sibling of their workgroup (render_body, "ray hand-over")
	uint32_t fill_lanes;       // small-launch schedule (all_tail): lanes that stand on one pixel during the fill (4, 2 or 1: packets of 16 / 32 / 64 pixels)
	uint32_t p_big;            // hybrid launches (team == 0): packets [0, p_big) are 8x8, the rest 4x4 tail packets; else 0
	uint32_t team;             // 0 = hybrid (full generations, lane teams for the queue's tail); lanes per ray: 1, or 2 / 4 for launches with too few rays to fill the GPU (render_kernel's TEAM)
	uint32_t spp_count;        // samples of the view in this launch's queue (nrs_render_nerf_spp; 1: a single frame): n_packets = spp_count * spp_packets and, hybrid, p_big = spp_count * spp_big
	uint32_t spp_packets;      // packets of ONE sample (what n_packets is for a single frame)
	uint32_t spp_big;          // hybrid launches: 8x8 packets of one sample (what p_big is for a single frame)
	uint32_t slab_stride;      // pixels from one sample's slab of frame / depth / steps to the next (0 for a single frame)
	uint32_t max_steps;
	uint32_t dbg;              // NRS_DEBUG ablation bits (profiling only; 0 in production): 1 = all gathers hit entry 0, 2 = skip the MLPs
	float*    frame;           // f32x4
	float*    depth;
	uint32_t* steps;           // nullable
	RenderCounters* counters;
	RenderCounters* counters_next; // the block the slot's NEXT launch will use: zeroed by this launch's last workgroup (nullable)
	unsigned long long* wave_log; // NRS_DEBUG & 4: 4 words per wave (see nrs_render_nerf)
	const nrs_sample_view* views; // nrs_render_nerf_spp_views: spp_count records in the launch slot's device table, sample s renders with record s (null: every sample with p's camera)
};

// kernel launchers (nrs_render.hip, nrs_network.hip, nrs_display.hip, nrs_tables.hip, nrs_occupancy.hip).  stream is a hipStream_t.
// launches row `row` of kRoutes (nrs_route.h; the caller planned it: plan_route), or its batch twin when a.spp_count > 1
int launch_render(RouteId row, const DeviceModel& m, const RenderArgs& a, int n_cus, void* stream);
// n records of a views batch into the launch slot's table, ordered on the stream; h_views is free when the call returns (the records travel as kernel arguments)
int launch_views_upload(const nrs_sample_view* h_views, uint32_t n, nrs_sample_view* d_views, void* stream);
unsigned long long launch_render_dispatches(); // render-kernel dispatches of this process so far (nrs_ctx_render_launches counts with it)
// render mode Slice (Testbed::render_nerf's branch, testbed_nerf.cu:3111-3175): one network evaluation per owned pixel on the slice plane
int launch_slice(const DeviceModel& m, const RenderArgs& a, int n_cus, void* stream);
int launch_trace_samples(const DeviceModel& m, const nrs_render_params& p, uint32_t n_pixels, const uint32_t* d_pixel_idx,
                         uint32_t max_samples, float* d_t, float* d_dt, uint32_t* d_count, void* stream);
// The operators of network_kernel on caller batches (its MODE template argument: an unscoped enum, so the kernels keep their `int` symbol names).
enum NetOp : int {
	kNetInference = 0,          // inference_mixed_precision: 16 channels, c3 = density raw
	kNetDensity = 1,            // density(): the density MLP's outputs
	kNetEncode = 2,             // the hash-grid features, fp16 [n x 32]
	kNetInputGradient = 3,      // input_gradient(stream, 3, ...): d density_raw / d position, f32 [n x 3]
	kNetVisualizeActivation = 4,// visualize_activation(vis_layer, vis_dim): f32 [n]
	kNetInferenceDeep = 5,      // kNetInference of a network with a third rgb hidden layer: the launcher's choice (DeviceModel::rgb_deep), never a caller's
};
// ld_out, layout: kNetInference / kNetDensity / kNetEncode only; vis_layer (a kernel layer: nrs_api_network.cpp kernel_layer), vis_dim: kNetVisualizeActivation only.
// per_sample_light: floats 7..9 of a record are that sample's warped light direction (a model with n_extra_dims = 3 and ld_in >= 10); else DeviceModel::light01
int launch_network(const DeviceModel& m, NetOp op, uint32_t n, const float* d_in, uint32_t ld_in, void* d_out, uint32_t ld_out,
                   int layout, int n_cus, void* stream, bool per_sample_light = false, uint32_t vis_layer = 0, uint32_t vis_dim = 0);
// NerfNetwork::backward for base.json's architecture at the default numerics (nrs_network_backward.hip): parameter gradients ADDED to d_dparams (fp32, the blob's order),
// optionally dL/dposition into floats 0..2 of d_dinput's records
int launch_network_backward(const DeviceModel& m, uint32_t n, const float* d_in, uint32_t ld_in, const void* d_dout, uint32_t ld_dout, int layout,
                            float* d_dparams, float* d_dinput, int n_cus, void* stream);
int launch_selection_rays(const DeviceModel& m, const nrs_render_params& p, const int32_t* d_pixels, uint32_t n, float threshold,
                          float* d_positions, uint32_t* d_cells, uint8_t* d_found, void* stream);
int launch_poisson_fit(const DeviceModel& m, uint32_t n_verts, uint32_t n_sh, const float* d_coords, const void* d_net, int is_inside, float scale,
                       float* d_density, float* d_sh, void* stream);
int launch_cell_records(const DeviceModel& m, uint32_t n_levels, void* d_records, void* stream);
int launch_weight_fragments(const uint16_t* d_params, const uint16_t* d_src, uint16_t* d_frag, uint32_t n, void* stream);
constexpr uint32_t kBrick = 8, kBrickCells = kBrick * kBrick * kBrick; // sparse cell records: 8^3 cells = 16 KiB of records per brick
// Order of the 512 records inside a brick.  0: x fastest (a 128-byte line = the 4 records of a 4 x 1 x 1 run of cells); 1: Morton (a line = a 2 x 2 x 1 block, two
// lines = 2 x 2 x 2): VERDICT r3 next #7's experiment -- measured on the aabb-16 scene in round 4, see HISTORY.md (round 4) / profiles/r04_garden.md.
#ifndef NRS_BRICK_MORTON
#define NRS_BRICK_MORTON 0
#endif
// position of cell (x, y, z) (each 0..7) among its brick's records -- shared by the kernel that writes the records and the gather that reads them
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t brick_slot(uint32_t x, uint32_t y, uint32_t z) {
#if NRS_BRICK_MORTON
	auto spread = [](uint32_t v) { return (v & 1u) | ((v & 2u) << 2) | ((v & 4u) << 4); };
	return spread(x) | (spread(y) << 1) | (spread(z) << 2);
#else
	return (z << 6) | (y << 3) | x;
#endif
}
int launch_brick_mark(const DeviceModel& m, const LevelParams& lp, const uint8_t* d_mask, uint32_t* d_table, uint32_t* d_counter, uint32_t* d_slots, uint32_t capacity, void* stream);
int launch_brick_fill(const DeviceModel& m, const LevelParams& lp, const uint32_t* d_slots, uint32_t n_bricks, void* d_records2, void* stream);
enum GridEvalOp : int { kGridDensity = 0, kGridRgba = 1 }; // get_density_on_grid / get_rgba_on_grid (grid_eval_kernel's MODE)
int launch_grid_eval(const DeviceModel& m, GridEvalOp op, const uint32_t res[3], const float box_mn[3], const float box_mx[3], const float dir01[3],
                     const float* d_density_grid, float* d_out, int n_cus, void* stream);
int launch_map_rays(const DeviceEdit& e, uint32_t n, float* d_coords, uint32_t ld, int with_dir, uint8_t* d_empty, void* stream);
int launch_grid_to_bitfield(const float* d_grid, uint8_t* d_bitfield, float* d_scratch_mean, void* stream);
// both flavours of the marching accelerator from the bitfield: d_masks 2 x kCoarseWords words; d_out 2 x {mn[3], mx[3], cell[3], inv_cell[3]}
// (slot 0: any step parameters, slot 1: cone_angle == 0 && min_mip == 0); d_keys: 12 words of scratch
int launch_occ_accel(const uint8_t* d_bitfield, uint32_t* d_masks, float* d_out, uint32_t* d_keys, void* stream);
// one iteration of update_density_grid_nerf_operator up to (not including) mean/bitfield; d_grid_tmp must be zeroed
int launch_grid_update(const DeviceModel& m, const DeviceEdit* d_edits, int n_edits, const nrs_grid_update& u, uint64_t rng_state_nonuniform,
                       float* d_grid, uint32_t* d_grid_tmp, int n_cus, void* stream);
int launch_accumulate(uint32_t n_pixels, const float* d_frame, float* d_accum, uint32_t sample_count, int color_space, void* stream);
int launch_accumulate_spp(uint32_t n_pixels, const float* d_frames, size_t slab_stride_pixels, uint32_t spp_count, float* d_accum, uint32_t sample_count, int color_space, void* stream);
// the display step (tonemap_kernel) and the last fold of a view fused with it; p has been validated by the caller (nrs_api_display.cpp: check_tonemap_params)
int launch_tonemap(uint32_t n_pixels, const float* d_accum, const nrs_tonemap_params& p, void* d_out, void* stream);
int launch_accumulate_spp_tonemap(uint32_t n_pixels, const float* d_frames, size_t slab_stride_pixels, uint32_t spp_count, float* d_accum, uint32_t sample_count,
                                  const nrs_tonemap_params& p, void* d_out, void* stream);
int launch_detile(const nrs_render_params& p, uint32_t n_ranks, size_t rank_stride_floats, const float* d_tiles, uint32_t channels,
                  float* d_image, void* stream);
const char* launch_last_error();

// The middle launch of a three-launch exclusive scan (nrs_scan.hip): d_sums [n_tiles][n_values] (n_values 1 or 2), one row per tile, becomes its exclusive prefix in
// place, in one workgroup, for any n_tiles; d_totals[n_values] = the sums of all tiles; *d_total_copy (nullable) = d_totals[0] again.
int launch_tile_scan(uint32_t n_tiles, uint32_t n_values, uint32_t* d_sums, uint32_t* d_totals, uint32_t* d_total_copy, void* stream);

// cage-move chain on the device (nrs_cage.hip)
constexpr uint32_t kLutScanTiles = kGridVol * kCascades / 4096;
constexpr uint32_t kFineMaxCells = 16u << 20; // fine look-up table: at most 16 M fine cells (64 MB of offsets) per edit; the subdivision is chosen to fit
constexpr uint32_t kFineScanTiles = kFineMaxCells / 4096;
constexpr int32_t kFinePlain = 0xff;          // DeviceEdit::fine_win[c][7]: no fine table for cascade c
constexpr int32_t kFineMaxList = 96;          // cascades whose longest LUT list exceeds this keep the plain scan (the coarse cascades of a small cage: hundreds of tets inside one cell,
                                              // hardly a sample; one wave of the build would walk such a list 64 fine cells wide -- 95 us at 285 tets)
constexpr uint32_t kFineHeadTetBits = 25;     // DeviceEdit::fine_head[cell].y: first tet | list length << 25 (an edit of 2^25 tets or more keeps no heads)
static_assert(kFineMaxList < (1 << (32 - kFineHeadTetBits)), "a fine list (a filtered LUT list of at most kFineMaxList tets) must fit the head word's length field");
int launch_mvc_apply(uint32_t n_points, uint32_t n_cv, const float* d_weights, const float* d_cage, float* d_points, void* stream);
int launch_bbox(uint32_t n, const float* d_verts, float* d_out6, void* stream);
int launch_poisson_interpolate(uint32_t n_points, uint32_t n_cv, const float* d_gamma, const float* d_per_cage, float* d_shs, float* d_out_density, float* d_res_density, void* stream);
int launch_lut_count_scan(uint32_t n_tets, const float* d_verts, const uint32_t* d_tets, uint32_t* d_counts, uint32_t* d_tile_sums,
                          uint32_t* d_offsets, uint32_t* d_total, unsigned long long* d_hit_masks /* [2 * n_tets * kCascades]: written */,
                          float cells0 /* estimate: cells of cascade 0 in a tet's bounding box (team size) */, void* stream);
int launch_lut_fill(uint32_t n_tets, const float* d_verts, const uint32_t* d_tets, uint32_t* d_counts, const uint32_t* d_offsets, uint32_t* d_idx,
                    uint8_t* d_bitfield, uint32_t* d_scratch_u32 /* 3 words */, uint32_t* d_big_cells, uint32_t n_work /* its entries */, unsigned long long* d_hit_masks /* as the count pass left them */, float cells0, void* stream);
uint32_t lut_big_list_capacity(size_t idx_capacity);
int launch_tet_planes(uint32_t n_tets, const float* d_verts, const uint32_t* d_tets, float* d_planes, void* stream);
// fine look-up table (DeviceEdit::fine_*): d_window_out[kCascades][8] = min x, y, z / max x, y, z of the LUT cells with a non-empty list (min > max: none), their number, the longest list
int launch_fine_window(const uint32_t* d_lut_off, int32_t* d_window_out, void* stream);
// counts (FILL = false: d_counts[n_padded], then the exclusive scan into d_fine_off[n_padded + 1] and *d_total) or fills (FILL = true: d_fine_idx) the fine lists of `de`'s windows
int launch_fine_count_scan(const DeviceEdit& de, uint32_t n_fine_cells, uint32_t* d_counts, uint32_t* d_tile_sums, uint32_t* d_fine_off, uint32_t* d_total, void* stream);
int launch_fine_fill(const DeviceEdit& de, uint32_t n_fine_cells, const uint32_t* d_fine_off, uint32_t* d_fine_idx, uint2* d_fine_head /* [fine cells]; nullable: no head words */, void* stream);
// d_mapback (nullable): the rotation part of the map-back records (DeviceEdit::mapback) is written with d_out
int launch_local_rotations(uint32_t n_tets, const float* d_verts, const float* d_orig, const uint32_t* d_tets, float* d_out, float* d_mapback, void* stream);
// the whole map-back record of every tet: canonical vertices, and the rotations d_rot holds now (null: zeros)
int launch_tet_mapback(uint32_t n_tets, const float* d_orig, const uint32_t* d_tets, const float* d_rot, float* d_mapback, void* stream);

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

// selection tool (nrs_selection.hip).  Morphology works on one level of a bitfield re-packed to x-major rows: word (z * 128 + y) * 4 + x / 32, bit x % 32.
constexpr uint32_t kMorphLevelWords = kGridVol / 32;
constexpr int32_t kMorphMaxRadius = 10;          // the reference's slider, correct_mm_operations.cu:16
constexpr uint32_t kMorphMaxTaps = (2 * kMorphMaxRadius + 1) * (2 * kMorphMaxRadius + 1);
// a structuring element as rows: tap i covers x - half[i] .. x + half[i] of row (y + dy[i], z + dz[i]); sorted by descending half.  invert: erosion (the walk runs on the complement)
struct MorphPlan {
	uint32_t n_taps, invert;
	int8_t dy[kMorphMaxTaps], dz[kMorphMaxTaps], half[kMorphMaxTaps];
};
int launch_morph_pack(const uint32_t* d_morton_level, uint32_t* d_rows, void* stream);
int launch_morph_unpack(const uint32_t* d_rows, uint32_t* d_morton_level, void* stream);
int launch_morph_rows(const MorphPlan& plan, const uint32_t* d_rows_in, uint32_t* d_rows_out, void* stream); // in != out
// [128^3] floats, x + 128 y + 128^2 z: 1.0 where the row bit is set and the cell is not on the grid's shell, else 0.0
int launch_selection_lattice(const uint32_t* d_rows, float* d_lattice, void* stream);

// The planner behind one C symbol (exported from libnrs.so, declared here only: not part of include/nrs.h): tests sweep it without a GPU.
struct RouteProbe {
	int32_t  status;
	int32_t  row;              // RouteId, -1 when refused
	uint32_t team, all_tail, fill_lanes, tail_every, tail_target, hybrid;
	uint32_t row_has_batch;
	char     name[96];         // the row as route_name prints it for this request (", batch" for spp_count > 1)
	char     message[256];
};

// the thread-local message nrs_last_error() returns (nrs_api.cpp); used by the host-only translation units
void set_last_error(const char* msg);

} // namespace nrs

// plans n requests; request_size / probe_size are the caller's sizeof of the two structs (a mirror that has drifted is refused: NRS_ERR_INVALID_ARG)
extern "C" int nrs_route_probe(const nrs::RouteRequest* requests, uint32_t request_size, uint32_t n, nrs::RouteProbe* out, uint32_t probe_size);
// RoutePlan::views of each request (0 for a refused one): what nrs_route_probe's answer has no field for
// (a second test-only export that plans every request again for one field: RouteProbe gets a `views` member, and this goes, when RouteProbe's mirrors next change)
extern "C" int nrs_route_probe_views(const nrs::RouteRequest* requests, uint32_t request_size, uint32_t n, uint32_t* views_out);
