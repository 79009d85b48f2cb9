// nrs_scan.h -- the launcher of nrs_scan.hip.
#pragma once
#include <stdint.h>

namespace nrs {

// The middle launch of a three-launch exclusive scan (nrs_scan.hip): d_sums [n_tiles][n_values] (n_values 1 or 2), one row per tile, becomes its exclusive prefix in
// place, in one workgroup, for any n_tiles; d_totals[n_values] = the sums of all tiles; *d_total_copy (nullable) = d_totals[0] again.
int launch_tile_scan(uint32_t n_tiles, uint32_t n_values, uint32_t* d_sums, uint32_t* d_totals, uint32_t* d_total_copy, void* stream);

} // namespace nrs
