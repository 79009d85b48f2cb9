// nrs_loss.cuh -- the per-channel loss of the training path and the colour curves it is evaluated behind, each stated once: the ray loss (nrs_train.hip), the
// environment map's gradient (nrs_envmap.hip) and the exposure's (nrs_exposure.hip) read the same text, so the same inputs give them the same bits.  (The fixed-point
// cells the two gradients are deposited in: nrs_cells.h.)
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/nrs.h"

namespace nrs {

// common_device.cuh:31-37, :43-49, :55-61, with powf: once per ray, and the loss is compared more tightly than a displayed colour
__device__ __forceinline__ float train_srgb_to_linear(float s) { return s <= 0.04045f ? s / 12.92f : powf((s + 0.055f) / 1.055f, 2.4f); }
__device__ __forceinline__ float train_srgb_to_linear_derivative(float s) { return s <= 0.04045f ? 1.0f / 12.92f : 2.4f / 1.055f * powf((s + 0.055f) / 1.055f, 1.4f); }
__device__ __forceinline__ float train_linear_to_srgb(float l) { return l < 0.0031308f ? 12.92f * l : 1.055f * powf(l, 0.41666f) - 0.055f; }

// loss_and_gradient (tn:173-185) of one channel: the seven functions of tn:103-171, Huber with alpha = 1
__device__ __forceinline__ void loss_and_gradient(uint32_t type, float target, float pred, float& loss, float& grad) {
	const float diff = pred - target;
	switch (type) {
		case NRS_LOSS_RELATIVE_L2: { const float f = 1.0f / (pred * pred + 1e-2f); loss = diff * diff * f; grad = 2.0f * diff * f; break; }
		case NRS_LOSS_L1: loss = fabsf(diff); grad = copysignf(1.0f, diff); break;
		case NRS_LOSS_MAPE: { const float f = 1.0f / (fabsf(pred) + 1e-2f); loss = fabsf(diff) * f; grad = copysignf(f, diff); break; }
		case NRS_LOSS_SMAPE: { const float f = 1.0f / (0.5f * (fabsf(pred) + fabsf(target)) + 1e-2f); loss = fabsf(diff) * f; grad = copysignf(f, diff); break; }
		case NRS_LOSS_HUBER: {
			const float ad = fabsf(diff);
			loss = ad > 1.0f ? ad - 0.5f : 0.5f * diff * diff;
			grad = ad > 1.0f ? (diff > 0 ? 1.0f : -1.0f) : diff;
			break;
		}
		case NRS_LOSS_LOG_L1: { const float div = fabsf(diff) + 1.0f; loss = logf(div); grad = copysignf(1.0f / div, diff); break; }
		default: loss = diff * diff; grad = 2.0f * diff; break; // L2
	}
}

} // namespace nrs
