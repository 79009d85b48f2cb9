// nrs_train.h -- what nrs_api_train.cpp and nrs_train.hip share: the argument blocks and launchers of the training-ray path (include/nrs.h, "training rays").
// Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/nrs.h"
#include "nrs_internal.h"

namespace nrs {

constexpr uint32_t kTrainMaxRays = 1u << 21; // 2^21 rays x NERF_STEPS = 2^31 samples: every sum of counts fits 32 bits
constexpr uint32_t kRayAuxWords = 12;        // nrs_ray_loss_ex's record per slot: g[3], T, target[3], C[3], n, M
constexpr uint32_t kTrainScanTile = 1024;    // rays per tile of the scan over the per-ray counts
// The live slots of a step: the generator's ray counter (nrs_training_samples' d_counters[0]), never more than n_rays.  Whatever is indexed by slot -- the loss, the
// environment map, the exposure, the error map -- stops here.
__device__ __forceinline__ uint32_t live_slots(const uint32_t* ray_counter, uint32_t n_rays) {
	const uint32_t emitted = *ray_counter;
	return emitted < n_rays ? emitted : n_rays;
}
inline uint32_t train_scan_tiles(uint32_t n_rays) { return (n_rays + kTrainScanTile - 1u) / kTrainScanTile; }
// what the scan keeps behind a view's per-ray arrays: two sums per tile, then the two totals
inline size_t train_scan_words(uint32_t n_rays) { return 2 * (size_t)train_scan_tiles(n_rays) + 2; }

// The per-ray workspace (the model owns it: nrs_model::d_train_ws) as each of its two users sees it: 32-bit words, arrays of n_rays, laid out in the order of the
// members, the scan's words last.  A view is built from (ws, n_rays) wherever it is needed.
struct TrainSamplesWs { // the generator
	uint32_t *count, *base, *slot; // [n_rays] each: samples of the ray, samples in front of it, rays with samples in front of it
	uint32_t* end;                 // one word: where the last emitted ray ends
	uint32_t* tiles;               // [train_scan_words]
	__host__ __device__ TrainSamplesWs(uint32_t* ws, uint32_t n) : count(ws), base(count + n), slot(base + n), end(slot + n), tiles(end + 1) {}
};
struct RayLossWs { // the loss
	uint32_t *M, *cbase;   // [n_rays] each: samples consumed, compact samples in front of the ray
	float *C[3], *g[3];    // [n_rays] each: the composited colour and dLoss/dC
	float* loss;           // [n_rays]: mean loss / n_rays
	uint32_t* tiles;       // [train_scan_words]
	__host__ __device__ RayLossWs(uint32_t* ws, uint32_t n) : M(ws), cbase(M + n) {
		float* f = reinterpret_cast<float*>(cbase + n);
		for (int k = 0; k < 3; ++k, f += n) C[k] = f;
		for (int k = 0; k < 3; ++k, f += n) g[k] = f;
		loss = f;
		tiles = reinterpret_cast<uint32_t*>(loss + n);
	}
};
// the words a view spans
template <class View>
inline size_t train_ws_words(uint32_t n_rays) {
	uint32_t* const ws = nullptr;
	return (size_t)(View(ws, n_rays).tiles - ws) + train_scan_words(n_rays);
}

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
	uint32_t* ws;            // TrainSamplesWs: train_ws_words<TrainSamplesWs>(n_rays) words (NULL when n_rays == 0)
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
	uint32_t* ws;                // RayLossWs: train_ws_words<RayLossWs>(n_rays) words (NULL when n_rays == 0)
	const float* background_linear; // nullable: [n_rays][3] by slot, replaces srgb_to_linear(background) (nrs_ray_loss_ex)
	uint32_t* ray_aux;           // nullable: [n_rays][kRayAuxWords], 16-byte aligned (nrs_ray_loss_ex)
};

int launch_training_samples(const DeviceModel& m, const TrainSamplesArgs& a, void* stream);
int launch_ray_loss(const DeviceModel& m, const RayLossArgs& a, void* stream);

} // namespace nrs
