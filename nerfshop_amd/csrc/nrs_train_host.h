// nrs_train_host.h -- what the training units behind the C-ABI share (nrs_api_train.cpp, nrs_api_optimizer.cpp, nrs_api_dataset.cpp, nrs_api_envmap.cpp,
// nrs_api_exposure.cpp), each stated ONCE: the refusals they word alike, and the way a handle's signed cells reach the host.  It sits on nrs_handles.h, so that the
// units that do not train read none of the training headers.  Host-only C++17: no .hip / .cuh includes it.
#pragma once
#include "nrs_handles.h"
#include "nrs_train.h"
#include "nrs_cells.h"

#include <cmath>

namespace nrs {

// `who` is the entry point's name, the prefix of its message.
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0u; }
// kTrainMaxRays: the sample counters are 32 bits wide, the generator draws no more, a fixed-point cell holds no more without a wrap -- `why` says which, in brackets
inline int check_ray_count(uint32_t n_rays, const char* who, const char* why = "") {
	if (n_rays > kTrainMaxRays) return fail(NRS_ERR_INVALID_ARG, std::string(who) + ": more than 2^21 rays" + why);
	return NRS_OK;
}
// an optimiser step's two scalars
inline int check_step_scalars(float loss_scale, float learning_rate, const char* who) {
	if (!std::isfinite(loss_scale) || !(loss_scale > 0.f)) return fail(NRS_ERR_INVALID_ARG, std::string(who) + ": loss_scale is not finite or <= 0");
	if (!std::isfinite(learning_rate) || learning_rate < 0.f) return fail(NRS_ERR_INVALID_ARG, std::string(who) + ": learning_rate is negative or not finite");
	return NRS_OK;
}

// A handle's signed cells (nrs_cells.h) to the host, for nrs_envmap_get and nrs_exposure_get once they have waited for the device: the cells themselves, int64, or --
// as_gradient -- the step's own expression on the cells as they are now, f32: the gradient the next step will read.
template <class Handle>
int signed_cells_to_host(Handle* e, size_t n, bool as_gradient, void* h_out) {
	if (!as_gradient) {
		HIP_TRY(hipMemcpy(h_out, e->d_cells.get(), n * sizeof(int64_t), hipMemcpyDeviceToHost));
		return NRS_OK;
	}
	std::vector<int64_t> cells(n);
	HIP_TRY(hipMemcpy(cells.data(), e->d_cells.get(), n * sizeof(int64_t), hipMemcpyDeviceToHost));
	signed_cells_to_float(cells.data(), n, (float*)h_out);
	return NRS_OK;
}

} // namespace nrs
