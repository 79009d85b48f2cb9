// nrs_exposure.h -- what nrs_api_exposure.cpp and nrs_exposure.hip share: the argument blocks and launchers of per-image exposure (include/nrs.h, "per-image
// exposure").  Not part of the public ABI.
#pragma once
#include "../../include/nrs.h"
#include "nrs_exposure_math.h"

namespace nrs {

struct ExposureTargetsArgs {
	uint32_t n_rays, n_images;
	const uint32_t* ray_counter;  // live slots, capped at n_rays
	const uint32_t* ray_indices;  // [n_rays]: the ray of a slot
	const uint32_t* pixels;       // [n_rays][2] by ray: (img, pixel)
	const float* target_rgba;     // [n_rays][4] by ray
	const float* exposure;        // [n_images][3]
	float* target_out;            // [n_rays][4] by slot
	uint32_t* scale;              // [n_rays][4] by slot, 16-byte aligned: the bits of scale.xyz, img
};

struct ExposureAccumulateArgs {
	uint32_t n_rays, n_images;
	const uint32_t* ray_counter;
	const uint32_t* ray_indices;
	const uint32_t* numsteps_out; // [n_rays][2]: nrs_ray_loss_ex's (M', cbase)
	const uint32_t* ray_aux;      // [n_rays][kRayAuxWords], 16-byte aligned
	const uint32_t* scale;        // what nrs_exposure_targets wrote
	const float* xy_pdf;          // nullable: [n_rays] by ray
	uint32_t train_in_linear_colors;
	float loss_scale;
	unsigned long long* cells;    // [n_images][3]: int64 as two's complement
};

struct ExposureStepArgs {
	uint32_t n_images;
	ExposureStepConsts k;
	unsigned long long* cells;
	float *values, *m, *v;
};

int launch_exposure_targets(const ExposureTargetsArgs& a, void* stream);
int launch_exposure_accumulate(const ExposureAccumulateArgs& a, void* stream);
int launch_exposure_step(const ExposureStepArgs& a, void* stream);

} // namespace nrs
