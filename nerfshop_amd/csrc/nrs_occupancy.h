// nrs_occupancy.h -- the launchers of nrs_occupancy.hip: bitfield, marching accelerator, occupancy refresh.
#pragma once
#include <stdint.h>
#include "../../include/nrs.h"
#include "nrs_internal.h"

namespace nrs {

int launch_grid_to_bitfield(const float* d_grid, uint8_t* d_bitfield, float* d_scratch_mean, void* stream);
// both flavours of the marching accelerator from the bitfield: d_masks 2 x kCoarseWords words; d_out 2 x {mn[3], mx[3], cell[3], inv_cell[3]}
// (slot 0: any step parameters, slot 1: cone_angle == 0 && min_mip == 0); d_keys: 12 words of scratch
int launch_occ_accel(const uint8_t* d_bitfield, uint32_t* d_masks, float* d_out, uint32_t* d_keys, void* stream);
// one iteration of update_density_grid_nerf_operator up to (not including) mean/bitfield; d_grid_tmp must be zeroed
int launch_grid_update(const DeviceModel& m, const DeviceEdit* d_edits, int n_edits, const nrs_grid_update& u, uint64_t rng_state_nonuniform,
                       float* d_grid, uint32_t* d_grid_tmp, int n_cus, void* stream);

} // namespace nrs
