// nrs_internal.h -- what SEVERAL subsystems share, host code and HIP kernels alike: the grid and fragment constants, the model and the edit operator as the kernels
// read them, the launch-error message.  A launcher, and a POD only it and its callers use, is declared in the header named after the .hip that defines it
// (nrs_render.h, nrs_network.h, nrs_cage.h, ...).  Nothing here is part of the public ABI (that is include/nrs.h).
#pragma once
#include <stdint.h>
#include <stddef.h>
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
const char* launch_last_error();

// the thread-local message nrs_last_error() returns (nrs_api.cpp); used by the host-only translation units
void set_last_error(const char* msg);

} // namespace nrs
