// nrs_exposure_math.h -- the arithmetic of per-image exposure's optimiser step (include/nrs.h, "per-image exposure"), stated ONCE for exposure_step_kernel
// (nrs_exposure.hip) and for its CPU twin (exposure_step_host below, behind nrs_exposure_step_host).  Plain C++ with <math.h> only.  Every expression is float32 in the
// written order; the translation units that include it are built with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>

#include "nrs_cells.h"

#if defined(__HIPCC__)
#define NRS_EXPOSURE_FN __host__ __device__ __forceinline__
#else
#define NRS_EXPOSURE_FN inline
#endif

namespace nrs {

constexpr float kExposureLn2 = 0.6931471805599453f;

// what the host works out once per step and every element reads
struct ExposureStepConsts {
	float beta1, beta2, epsilon, l2_reg;
	float pcls; // per_camera_loss_scale = (float)n_images / loss_scale / (float)steps_between_updates (tn:3838)
	float alr;  // learning_rate * sqrt(1 - beta2^t) / (1 - beta1^t) in float64, rounded once
};

inline ExposureStepConsts exposure_step_consts(uint32_t n_images, float beta1, float beta2, float epsilon, float l2_reg, uint32_t steps_between_updates, float loss_scale,
                                               float learning_rate, uint32_t t) {
	ExposureStepConsts k;
	k.beta1 = beta1; k.beta2 = beta2; k.epsilon = epsilon; k.l2_reg = l2_reg;
	k.pcls = (float)n_images / loss_scale / (float)steps_between_updates;
	k.alr = (float)((double)learning_rate * sqrt(1.0 - pow((double)beta2, (double)t)) / (1.0 - pow((double)beta1, (double)t)));
	return k;
}

// adam_optimizer.h:41-44 on one channel of one image (tn:3892-3898): an element whose cell is zero still steps
NRS_EXPOSURE_FN void exposure_adam(const ExposureStepConsts& k, long long cell, float& value, float& m, float& v) {
	const float g = signed_cell_to_float(cell) * k.pcls + value * k.l2_reg;
	m = k.beta1 * m + (1.0f - k.beta1) * g;
	v = k.beta2 * v + (1.0f - k.beta2) * (g * g);
	value -= k.alr * (m / (sqrtf(v) + k.epsilon));
}
// The renormalisation's mean (tn:3900-3903) is a float64 sum in ONE fixed order, the kernel's and the twin's: kExposureMeanLanes strided partial sums -- partial j
// adds the images j, j + kExposureMeanLanes, ... in rising order, from 0.0 -- and then the partials in rising order, from 0.0.  (Up to kExposureMeanLanes images that
// is the sum over the images in their order.)
constexpr uint32_t kExposureMeanLanes = 1024; // the threads of exposure_step_kernel's one workgroup
NRS_EXPOSURE_FN double exposure_sum_partials(const double* partial) {
	double sum = 0.0;
	for (uint32_t j = 0; j < kExposureMeanLanes; ++j) sum += partial[j];
	return sum;
}
NRS_EXPOSURE_FN float exposure_mean(double sum, uint32_t n_images) { return (float)(sum / (double)n_images); }

// the whole step on host arrays: cells [3 n] int64 -> 0, values / m / v [3 n] f32 in place
inline void exposure_step_host(uint32_t n_images, const ExposureStepConsts& k, int64_t* cells, float* values, float* m, float* v) {
	const size_t n = 3 * (size_t)n_images;
	for (size_t e = 0; e < n; ++e) {
		exposure_adam(k, (long long)cells[e], values[e], m[e], v[e]);
		cells[e] = 0;
	}
	double partial[kExposureMeanLanes];
	for (int c = 0; c < 3; ++c) {
		for (uint32_t j = 0; j < kExposureMeanLanes; ++j) {
			partial[j] = 0.0;
			for (uint32_t i = j; i < n_images; i += kExposureMeanLanes) partial[j] += (double)values[3 * (size_t)i + c];
		}
		const float mean = exposure_mean(exposure_sum_partials(partial), n_images);
		for (uint32_t i = 0; i < n_images; ++i) values[3 * (size_t)i + c] -= mean;
	}
}

} // namespace nrs
