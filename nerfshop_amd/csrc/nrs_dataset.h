// nrs_dataset.h -- what nrs_api_dataset.cpp and nrs_dataset.hip share: the camera record as the device reads it and the launchers of the dataset's three kernels
// (include/nrs.h, "the dataset").  Not part of the public ABI.
#pragma once
#include "nrs_internal.h"

namespace nrs {

// One camera on the device: nrs_training_camera without its struct_size, 40 words.
//   [0..11] xform_start | [12..23] xform_end | [24..25] focal_length | [26..27] principal_point | [28..31] rolling_shutter | [32] distortion_mode (bits) | [33..39] params
constexpr uint32_t kCameraWords = 40;
static_assert(sizeof(nrs_training_camera) == (kCameraWords + 1) * 4, "the device record is the public struct behind its struct_size");

struct DatasetRaysArgs {
	uint32_t n_rays, n_rays_total, n_images, width, height;
	uint64_t rng_state, rng_inc;
	uint32_t snap, random_bg;
	const uint64_t* images;   // [n_images][height][width] fp16 RGBA
	const float* cameras;     // [n_images][kCameraWords]
	float* rays;              // [n_rays][6]
	float* jitter;            // [n_rays]
	float* target;            // [n_rays][4]
	float* background;        // [n_rays][3], written when random_bg
	uint32_t* pixels;         // [n_rays][2] or NULL
};

// `src` is on the device; format / flags / mask_color as nrs_dataset_set_image (the fp16 format never comes here: it is a copy)
int launch_dataset_convert(int format, const void* src, uint64_t* dst, uint64_t n_pixels, uint32_t flags, uint32_t mask_color, void* stream);
int launch_dataset_rays(const DatasetRaysArgs& a, void* stream);
int launch_mark_untrained(float* d_grid, uint32_t n_images, const float* d_cameras, uint32_t width, uint32_t height, int clear_visible, void* stream);

} // namespace nrs
