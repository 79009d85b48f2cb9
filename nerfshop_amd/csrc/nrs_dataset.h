// nrs_dataset.h -- what nrs_api_dataset.cpp and nrs_dataset.hip share: the camera record as the device reads it and the launchers of the dataset's kernels
// (include/nrs.h, "the dataset").  Not part of the public ABI.
#pragma once
#include "../../include/nrs.h"

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
	// what only dataset_rays_kernel<true> (nrs_dataset_rays_ex) reads: the two switches, the CDFs of the last build with their resolution, the two further outputs
	uint32_t by_images, by_pixels, cdf_res_x, cdf_res_y;
	const float* cdf_x_cond_y; // [n_images][cdf_res_y][cdf_res_x]
	const float* cdf_y;        // [n_images][cdf_res_y]
	const float* cdf_img;      // [n_images]
	float* xy;                 // [n_rays][2] or NULL
	float* pdf;                // [n_rays] or NULL
};

// the error map's deposits (include/nrs.h, "the training error map")
struct ErrorMapAccumulateArgs {
	uint32_t n_rays, n_images, res_x, res_y;
	const uint32_t* ray_counter;  // [1]
	const uint32_t* ray_indices;  // [n_rays], by slot
	const float* loss;            // [n_rays], by slot
	const float* xy;              // [n_rays][2], by ray
	const uint32_t* pixels;       // [n_rays][2], by ray
	const float* pdf;             // [n_rays] by ray, or NULL
	float* loss_weighted;         // [n_rays] by slot, NULL, or loss itself
	uint64_t* cells;              // [n_images][res_y][res_x]
};

// `src` is on the device; format / flags / mask_color as nrs_dataset_set_image (the fp16 format never comes here: it is a copy)
int launch_dataset_convert(int format, const void* src, uint64_t* dst, uint64_t n_pixels, uint32_t flags, uint32_t mask_color, void* stream);
int launch_dataset_rays(const DatasetRaysArgs& a, void* stream);
int launch_dataset_rays_ex(const DatasetRaysArgs& a, void* stream);
int launch_error_map_accumulate(const ErrorMapAccumulateArgs& a, void* stream);
// cdf_x_cond_y, cdf_y, img_total (the pictures' unnormalised totals), cdf_img and pmf_img from the cells
int launch_error_map_cdfs(uint32_t n_images, uint32_t res_y, uint32_t res_x, const uint64_t* d_cells, float* d_cdf_x_cond_y, float* d_cdf_y, float* d_img_total,
                          float* d_cdf_img, float* d_pmf_img, void* stream);
int launch_mark_untrained(float* d_grid, uint32_t n_images, const float* d_cameras, uint32_t width, uint32_t height, int clear_visible, void* stream);

} // namespace nrs
