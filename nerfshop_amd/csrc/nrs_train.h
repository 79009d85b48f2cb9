// nrs_train.h -- what nrs_api_train.cpp and nrs_train.hip share: the argument blocks and launchers of the training-ray path (include/nrs.h, "training rays").
// Not part of the public ABI.
#pragma once
#include "nrs_internal.h"

namespace nrs {

// Per-ray workspace, in 32-bit words, structure of arrays over n_rays (the model owns it: nrs_model::d_train_ws).
//   generator: count | base | slot, then one word: the end of the last emitted ray
//   ray loss:  M | cbase | C[3] | g[3] | mean loss / n_rays
// Behind the per-ray arrays: the generator's `end` word, then the scan's tile sums, 2 per 1024 rays, and its 2 totals.
constexpr uint32_t kTrainSamplesWsWords = 3;
constexpr uint32_t kRayLossWsWords = 9;
inline uint32_t train_scan_tiles(uint32_t n_rays) { return (n_rays + 1023u) / 1024u; }
inline size_t train_ws_words(uint32_t per_ray, uint32_t n_rays) { return (size_t)per_ray * n_rays + 1 + 2 * (size_t)train_scan_tiles(n_rays) + 2; }
constexpr uint32_t kTrainMaxRays = 1u << 21; // 2^21 rays x NERF_STEPS = 2^31 samples: every sum of counts fits 32 bits

struct TrainSamplesArgs {
	uint32_t n_rays;
	const float* rays;       // [n_rays][6]
	const float* jitter;     // [n_rays] or NULL
	float cone;
	uint32_t max_samples;
	float* coords;           // [max_samples][ld]
	uint32_t ld;
	uint32_t* numsteps;      // [n_rays][2]
	uint32_t* ray_indices;   // [n_rays]
	uint32_t* counters;      // [2]
	uint32_t* ws;            // train_ws_words(kTrainSamplesWsWords, n_rays) words (NULL when n_rays == 0)
};

struct RayLossArgs {
	nrs_ray_loss_params p;
	uint32_t n_rays;
	const uint32_t* ray_counter; // nullable
	const uint32_t* numsteps;
	uint32_t n_samples;
	const float* coords;
	uint32_t ld_in;
	const void* output;          // fp16
	uint32_t ld_out;
	int out_layout;
	const float* target_rgba;
	const float* background;     // nullable
	const float* origins;        // nullable
	uint32_t* numsteps_out;
	float* coords_out;
	void* dl;                    // fp16
	uint32_t ld_dl;
	int dl_layout;
	float* loss;                 // nullable
	uint32_t* counter_out;
	uint32_t* ws;                // train_ws_words(kRayLossWsWords, n_rays) words (NULL when n_rays == 0)
};

int launch_training_samples(const DeviceModel& m, const TrainSamplesArgs& a, void* stream);
int launch_ray_loss(const DeviceModel& m, const RayLossArgs& a, void* stream);

} // namespace nrs
