// nrs_envmap.h -- what nrs_api_envmap.cpp and nrs_envmap.hip share: the argument blocks and launchers of the trainable environment map (include/nrs.h, "the
// environment map").  Not part of the public ABI.
#pragma once
#include "../../include/nrs.h"

namespace nrs {

constexpr size_t kEnvmapMaxParams = 1ull << 31;  // 4 floats per texel; the optimiser's own limit (kAdamMaxParams)

struct EnvmapBackgroundArgs {
	uint32_t n_rays;
	const uint32_t* ray_counter;  // live slots, capped at n_rays
	const uint32_t* ray_indices;  // [n_rays]: the ray of a slot
	const float* rays;            // [n_rays][6] by ray
	const float* background;      // nullable: [n_rays][3] by slot, sRGB-encoded
	float default_background[3];  // sRGB-encoded, used when background is NULL
	const float* texels;          // [res_y][res_x][4], the live texels
	int32_t res[2];
	float* background_linear;     // [n_rays][3] by slot
	int32_t* footprint;           // [n_rays][4] by slot, 16-byte aligned: tx, ty, bits of wx, bits of wy
};

struct EnvmapAccumulateArgs {
	uint32_t n_rays;
	const uint32_t* ray_counter;
	const uint32_t* numsteps_out; // [n_rays][2]: nrs_ray_loss_ex's (M', cbase)
	const uint32_t* ray_aux;      // [n_rays][kRayAuxWords], 16-byte aligned
	const float* background_linear;
	const int32_t* footprint;     // 16-byte aligned
	uint32_t loss_type, envmap_loss_type, train_in_linear_colors;
	float loss_scale;
	int32_t res[2];
	unsigned long long* cells;    // [res_y][res_x][4]: int64 as two's complement
};

int launch_envmap_background(const EnvmapBackgroundArgs& a, void* stream);
int launch_envmap_accumulate(const EnvmapAccumulateArgs& a, void* stream);
// grad[i] = (float)((double)cell[i] * 2^-32) for every i < n, and 0 into every cell that was read non-zero
int launch_envmap_cells_to_gradient(uint32_t n, unsigned long long* cells, float* grad, void* stream);

} // namespace nrs
