// nrs_api_exposure.cpp -- per-image exposure behind the C-ABI (include/nrs.h, "per-image exposure"): the handle, its values and moments, the scaled target of a
// training ray, the gradient's deposits, the step and the step's host twin.  Everything that can be refused is refused before the first HIP call; targets, accumulate,
// step and export never wait for the device.
#include "nrs_train_host.h"
#include "nrs_exposure.h"
#include "nrs_train.h"

#include <cmath>
#include <new>

using namespace nrs;

namespace {

nrs_exposure_params default_exposure_params() {
	nrs_exposure_params p{};
	p.struct_size = sizeof(nrs_exposure_params);
	p.beta1 = 0.9f; p.beta2 = 0.99f; p.epsilon = 1e-8f; p.l2_reg = 0.0f; p.steps_between_updates = 16u;
	return p;
}

int check_params(const nrs_exposure_params* p, uint32_t n_images, const char* who) {
	const std::string w(who);
	if (n_images == 0u || n_images > NRS_EXPOSURE_MAX_IMAGES) return fail(NRS_ERR_INVALID_ARG, w + ": n_images is 0 or above 2^20");
	if (!p) return NRS_OK;
	if (p->struct_size != sizeof(nrs_exposure_params)) return fail(NRS_ERR_INVALID_ARG, w + ": params->struct_size is not sizeof(nrs_exposure_params)");
	if (!(p->beta1 >= 0.f && p->beta1 < 1.f)) return fail(NRS_ERR_INVALID_ARG, w + ": beta1 is outside [0, 1)");
	if (!(p->beta2 >= 0.f && p->beta2 < 1.f)) return fail(NRS_ERR_INVALID_ARG, w + ": beta2 is outside [0, 1)");
	if (!std::isfinite(p->epsilon) || !(p->epsilon > 0.f)) return fail(NRS_ERR_INVALID_ARG, w + ": epsilon is not finite or <= 0");
	if (!std::isfinite(p->l2_reg) || p->l2_reg < 0.f) return fail(NRS_ERR_INVALID_ARG, w + ": l2_reg is negative or not finite");
	if (p->steps_between_updates == 0u) return fail(NRS_ERR_INVALID_ARG, w + ": steps_between_updates is 0");
	return NRS_OK;
}

int zero_state(nrs_exposure* e, bool values_too) {
	const size_t n = 3 * (size_t)e->n_images;
	if (values_too) HIP_TRY(hipMemset(e->d_values.get(), 0, n * sizeof(float)));
	HIP_TRY(hipMemset(e->d_m.get(), 0, n * sizeof(float)));
	HIP_TRY(hipMemset(e->d_v.get(), 0, n * sizeof(float)));
	HIP_TRY(hipMemset(e->d_cells.get(), 0, n * sizeof(unsigned long long)));
	e->step_count = 0;
	e->rays_accumulated = 0;
	return NRS_OK;
}

} // namespace

extern "C" {

void nrs_exposure_default_params(nrs_exposure_params* out) {
	if (out) *out = default_exposure_params();
}

int nrs_exposure_create(nrs_ctx* ctx, uint32_t n_images, const nrs_exposure_params* params, nrs_exposure** out) {
	if (!ctx || !out) return fail(NRS_ERR_INVALID_ARG, "nrs_exposure_create: NULL argument");
	NRS_TRY(check_params(params, n_images, "nrs_exposure_create"));
	nrs_exposure* e = new (std::nothrow) nrs_exposure();
	if (!e) return fail(NRS_ERR_STATE, "out of host memory");
	e->ctx = ctx; e->n_images = n_images; e->p = params ? *params : default_exposure_params();
	const size_t n = 3 * (size_t)n_images;
	hipError_t he = hipSetDevice(ctx->device);
	if (he == hipSuccess) he = e->d_values.alloc(n);
	if (he == hipSuccess) he = e->d_m.alloc(n);
	if (he == hipSuccess) he = e->d_v.alloc(n);
	if (he == hipSuccess) he = e->d_cells.alloc(n);
	int status = he == hipSuccess ? NRS_OK : fail_hip(he, "nrs_exposure_create: device allocation");
	if (status == NRS_OK) status = zero_state(e, true);
	if (status == NRS_OK) {
		he = hipDeviceSynchronize();
		if (he != hipSuccess) status = fail_hip(he, "nrs_exposure_create: hipDeviceSynchronize");
	}
	if (status != NRS_OK) {
		nrs_exposure_destroy(e);
		return status;
	}
	*out = e;
	return NRS_OK;
}

void nrs_exposure_destroy(nrs_exposure* e) { delete e; } // (its buffers go with it)

uint32_t nrs_exposure_n_images(const nrs_exposure* e) { return e ? e->n_images : 0u; }
uint32_t nrs_exposure_step_count(const nrs_exposure* e) { return e ? e->step_count : 0u; }

int nrs_exposure_set(nrs_exposure* e, const float* h_values) {
	if (!e) return fail(NRS_ERR_INVALID_ARG, "nrs_exposure_set: NULL exposure");
	HIP_TRY(hipSetDevice(e->ctx->device));
	HIP_TRY(hipDeviceSynchronize()); // (steps in flight write what is reset here)
	NRS_TRY(zero_state(e, h_values == nullptr));
	if (h_values) HIP_TRY(hipMemcpy(e->d_values.get(), h_values, 3 * (size_t)e->n_images * sizeof(float), hipMemcpyHostToDevice));
	HIP_TRY(hipDeviceSynchronize());
	return NRS_OK;
}

int nrs_exposure_get(nrs_exposure* e, int which, void* h_out, size_t n) {
	if (which < NRS_EXPOSURE_VALUES || which > NRS_EXPOSURE_GRADIENT) return fail(NRS_ERR_INVALID_ARG, "nrs_exposure_get: unknown `which`");
	if (!e || !h_out) return fail(NRS_ERR_INVALID_ARG, "nrs_exposure_get: NULL argument");
	if (n != 3 * (size_t)e->n_images) return fail(NRS_ERR_INVALID_ARG, "nrs_exposure_get: n is not 3 * n_images");
	HIP_TRY(hipSetDevice(e->ctx->device));
	HIP_TRY(hipDeviceSynchronize());
	if (which == NRS_EXPOSURE_CELLS || which == NRS_EXPOSURE_GRADIENT) return signed_cells_to_host(e, n, which == NRS_EXPOSURE_GRADIENT, h_out);
	const float* src = which == NRS_EXPOSURE_VALUES ? e->d_values.get() : (which == NRS_EXPOSURE_M ? e->d_m.get() : e->d_v.get());
	HIP_TRY(hipMemcpy(h_out, src, n * sizeof(float), hipMemcpyDeviceToHost));
	return NRS_OK;
}

int nrs_exposure_export(nrs_exposure* e, float* d_out, void* stream) {
	if (!e || !d_out) return fail(NRS_ERR_INVALID_ARG, "nrs_exposure_export: NULL argument");
	HIP_TRY(hipSetDevice(e->ctx->device));
	HIP_TRY(hipMemcpyAsync(d_out, e->d_values.get(), 3 * (size_t)e->n_images * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
	return NRS_OK;
}

int nrs_exposure_targets(nrs_exposure* e, void* stream, uint32_t n_rays, const uint32_t* d_ray_counter, const uint32_t* d_ray_indices, const uint32_t* d_pixels,
                         const float* d_target_rgba, float* d_target_out, uint32_t* d_scale) {
	if (!e || (n_rays && (!d_ray_counter || !d_ray_indices || !d_pixels || !d_target_rgba || !d_target_out || !d_scale)))
		return fail(NRS_ERR_INVALID_ARG, "nrs_exposure_targets: NULL argument");
	NRS_TRY(check_ray_count(n_rays, "nrs_exposure_targets"));
	if (!aligned16(d_scale)) return fail(NRS_ERR_INVALID_ARG, "nrs_exposure_targets: d_scale is not 16-byte aligned");
	if (n_rays == 0) return NRS_OK;
	{ // one slot's output must not land on another slot's input: the two arrays are indexed differently
		const uintptr_t in = (uintptr_t)d_target_rgba, out = (uintptr_t)d_target_out, bytes = (uintptr_t)n_rays * 4u * sizeof(float);
		if (in < out + bytes && out < in + bytes) return fail(NRS_ERR_INVALID_ARG, "nrs_exposure_targets: d_target_out aliases d_target_rgba");
	}
	HIP_TRY(hipSetDevice(e->ctx->device));
	ExposureTargetsArgs a{};
	a.n_rays = n_rays; a.n_images = e->n_images; a.ray_counter = d_ray_counter; a.ray_indices = d_ray_indices; a.pixels = d_pixels; a.target_rgba = d_target_rgba;
	a.exposure = e->d_values.get(); a.target_out = d_target_out; a.scale = d_scale;
	NRS_LAUNCH(launch_exposure_targets(a, stream));
	return NRS_OK;
}

int nrs_exposure_accumulate(nrs_exposure* e, void* stream, const nrs_exposure_accumulate_params* p, uint32_t n_rays, const uint32_t* d_ray_counter,
                            const uint32_t* d_ray_indices, const uint32_t* d_numsteps_out, const uint32_t* d_ray_aux, const uint32_t* d_scale, const float* d_xy_pdf) {
	if (!e || !p || (n_rays && (!d_ray_counter || !d_ray_indices || !d_numsteps_out || !d_ray_aux || !d_scale)))
		return fail(NRS_ERR_INVALID_ARG, "nrs_exposure_accumulate: NULL argument");
	if (p->struct_size != sizeof(nrs_exposure_accumulate_params))
		return fail(NRS_ERR_INVALID_ARG, "nrs_exposure_accumulate: params->struct_size is not sizeof(nrs_exposure_accumulate_params)");
	if (!std::isfinite(p->loss_scale) || !(p->loss_scale > 0.f)) return fail(NRS_ERR_INVALID_ARG, "nrs_exposure_accumulate: loss_scale is not finite or <= 0");
	NRS_TRY(check_ray_count(n_rays, "nrs_exposure_accumulate"));
	if (!aligned16(d_ray_aux) || !aligned16(d_scale)) return fail(NRS_ERR_INVALID_ARG, "nrs_exposure_accumulate: d_ray_aux or d_scale is not 16-byte aligned");
	if (n_rays == 0) return NRS_OK;
	if (n_rays > kTrainMaxRays - e->rays_accumulated)
		return fail(NRS_ERR_STATE, "nrs_exposure_accumulate: more than 2^21 rays since the last nrs_exposure_step (the cells could wrap)");
	HIP_TRY(hipSetDevice(e->ctx->device));
	ExposureAccumulateArgs a{};
	a.n_rays = n_rays; a.n_images = e->n_images; a.ray_counter = d_ray_counter; a.ray_indices = d_ray_indices; a.numsteps_out = d_numsteps_out; a.ray_aux = d_ray_aux;
	a.scale = d_scale; a.xy_pdf = d_xy_pdf; a.train_in_linear_colors = p->train_in_linear_colors ? 1u : 0u; a.loss_scale = p->loss_scale;
	a.cells = e->d_cells.get();
	NRS_LAUNCH(launch_exposure_accumulate(a, stream));
	e->rays_accumulated += n_rays;
	return NRS_OK;
}

int nrs_exposure_step(nrs_exposure* e, void* stream, float loss_scale, float learning_rate) {
	if (!e) return fail(NRS_ERR_INVALID_ARG, "nrs_exposure_step: NULL exposure");
	NRS_TRY(check_step_scalars(loss_scale, learning_rate, "nrs_exposure_step"));
	HIP_TRY(hipSetDevice(e->ctx->device));
	ExposureStepArgs a{};
	a.n_images = e->n_images;
	a.k = exposure_step_consts(e->n_images, e->p.beta1, e->p.beta2, e->p.epsilon, e->p.l2_reg, e->p.steps_between_updates, loss_scale, learning_rate, e->step_count + 1u);
	a.cells = e->d_cells.get(); a.values = e->d_values.get(); a.m = e->d_m.get(); a.v = e->d_v.get();
	NRS_LAUNCH(launch_exposure_step(a, stream));
	e->step_count += 1u;
	e->rays_accumulated = 0;
	return NRS_OK;
}

int nrs_exposure_step_host(uint32_t n_images, const nrs_exposure_params* params, float loss_scale, float learning_rate, int64_t* cells, float* values, float* m, float* v,
                           uint32_t* step_count) {
	if (!cells || !values || !m || !v || !step_count) return fail(NRS_ERR_INVALID_ARG, "nrs_exposure_step_host: NULL argument");
	NRS_TRY(check_params(params, n_images, "nrs_exposure_step_host"));
	NRS_TRY(check_step_scalars(loss_scale, learning_rate, "nrs_exposure_step_host"));
	const nrs_exposure_params p = params ? *params : default_exposure_params();
	*step_count += 1u;
	exposure_step_host(n_images, exposure_step_consts(n_images, p.beta1, p.beta2, p.epsilon, p.l2_reg, p.steps_between_updates, loss_scale, learning_rate, *step_count), cells,
	                   values, m, v);
	return NRS_OK;
}

} // extern "C"
