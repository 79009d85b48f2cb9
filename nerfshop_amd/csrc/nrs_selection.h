// nrs_selection.h -- the launchers of nrs_selection.hip and the structuring element they take.
#pragma once
#include <stdint.h>
#include "nrs_internal.h"

namespace nrs {

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

} // namespace nrs
