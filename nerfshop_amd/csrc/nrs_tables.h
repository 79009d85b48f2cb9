// nrs_tables.h -- the launchers of nrs_tables.hip: cell records, weight fragments, brick tables, map_rays on caller batches.
#pragma once
#include <stdint.h>
#include "nrs_internal.h"

namespace nrs {

int launch_cell_records(const DeviceModel& m, uint32_t n_levels, void* d_records, void* stream);
int launch_weight_fragments(const uint16_t* d_params, const uint16_t* d_src, uint16_t* d_frag, uint32_t n, void* stream);
int launch_brick_mark(const DeviceModel& m, const LevelParams& lp, const uint8_t* d_mask, uint32_t* d_table, uint32_t* d_counter, uint32_t* d_slots, uint32_t capacity, void* stream);
int launch_brick_fill(const DeviceModel& m, const LevelParams& lp, const uint32_t* d_slots, uint32_t n_bricks, void* d_records2, void* stream);
int launch_map_rays(const DeviceEdit& e, uint32_t n, float* d_coords, uint32_t ld, int with_dir, uint8_t* d_empty, void* stream);

} // namespace nrs
