// nrs_display.h -- the launchers of nrs_display.hip: accumulate, tonemap, detile.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/nrs.h"

namespace nrs {

int launch_accumulate(uint32_t n_pixels, const float* d_frame, float* d_accum, uint32_t sample_count, int color_space, void* stream);
int launch_accumulate_spp(uint32_t n_pixels, const float* d_frames, size_t slab_stride_pixels, uint32_t spp_count, float* d_accum, uint32_t sample_count, int color_space, void* stream);
// the display step (tonemap_kernel) and the last fold of a view fused with it; p has been validated by the caller (nrs_api_display.cpp: check_tonemap_params)
int launch_tonemap(uint32_t n_pixels, const float* d_accum, const nrs_tonemap_params& p, void* d_out, void* stream);
int launch_accumulate_spp_tonemap(uint32_t n_pixels, const float* d_frames, size_t slab_stride_pixels, uint32_t spp_count, float* d_accum, uint32_t sample_count,
                                  const nrs_tonemap_params& p, void* d_out, void* stream);
int launch_detile(const nrs_render_params& p, uint32_t n_ranks, size_t rank_stride_floats, const float* d_tiles, uint32_t channels,
                  float* d_image, void* stream);

} // namespace nrs
