// nrs_cage.h -- the cage-move chain on the device (nrs_cage.hip): its launchers and the constants of the look-up tables they build.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <hip/hip_vector_types.h>
#include "nrs_internal.h"

namespace nrs {

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

} // namespace nrs
