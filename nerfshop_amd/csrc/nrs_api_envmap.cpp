// nrs_api_envmap.cpp -- the trainable environment map behind the C-ABI (include/nrs.h, "the environment map"): the handle, its texels and their optimiser, the
// background of a training ray, the gradient's deposits and the step.  Everything that can be refused is refused before the first HIP call; background, accumulate, step
// and export never wait for the device.
#include "nrs_train_host.h"
#include "nrs_envmap.h"
#include "nrs_train.h"

#include <cmath>
#include <new>

using namespace nrs;

namespace {

// base.json's "envmap" optimiser: Ema(0.99) over Adam(0.9, 0.99, 1e-10); no matrix weights, so l2_reg never acts
nrs_adam_params default_envmap_adam() {
	nrs_adam_params p{};
	p.struct_size = sizeof(nrs_adam_params);
	p.beta1 = 0.9f; p.beta2 = 0.99f; p.epsilon = 1e-10f; p.l2_reg = 0.0f; p.non_matrix_lr_factor = 1.0f; p.ema_decay = 0.99f;
	return p;
}

} // namespace

extern "C" {

void nrs_envmap_default_adam_params(nrs_adam_params* out) {
	if (out) *out = default_envmap_adam();
}

int nrs_envmap_create(nrs_ctx* ctx, uint32_t res_x, uint32_t res_y, const nrs_adam_params* params, nrs_envmap** out) {
	if (!ctx || !out) return fail(NRS_ERR_INVALID_ARG, "nrs_envmap_create: NULL argument");
	if (res_x < 1u || res_y < 1u) return fail(NRS_ERR_INVALID_ARG, "nrs_envmap_create: a resolution below 1 x 1");
	if ((uint64_t)res_x * res_y * 4u > kEnvmapMaxParams || res_x > 0x7fffffffu || res_y > 0x7fffffffu)
		return fail(NRS_ERR_INVALID_ARG, "nrs_envmap_create: more than 2^31 texel channels (4 * res_x * res_y)");
	if (params && params->struct_size != sizeof(nrs_adam_params)) return fail(NRS_ERR_INVALID_ARG, "nrs_envmap_create: params->struct_size is not sizeof(nrs_adam_params)");
	const nrs_adam_params p = params ? *params : default_envmap_adam();
	nrs_envmap* e = new (std::nothrow) nrs_envmap();
	if (!e) return fail(NRS_ERR_STATE, "out of host memory");
	e->ctx = ctx; e->res_x = res_x; e->res_y = res_y; e->n = 4u * res_x * res_y;
	int status = nrs_optimizer_create(ctx, e->n, 0, &p, &e->opt); // (refuses the remaining fields of params before its first HIP call, and selects the device)
	if (status == NRS_OK) {
		hipError_t he = e->d_grad.alloc(e->n);
		if (he == hipSuccess) he = e->d_cells.alloc(e->n);
		if (he == hipSuccess) he = hipMemset(e->d_grad.get(), 0, (size_t)e->n * sizeof(float));
		if (he == hipSuccess) he = hipMemset(e->d_cells.get(), 0, (size_t)e->n * sizeof(unsigned long long));
		if (he != hipSuccess) status = fail_hip(he, "nrs_envmap_create: device allocation");
	}
	// a fresh map is all zeros (this library's rule: the reference's initial values are tiny-cuda-nn's)
	if (status == NRS_OK) status = nrs_optimizer_set_weights(e->opt, e->d_grad.get(), 1, nullptr);
	if (status == NRS_OK) {
		const hipError_t he = hipStreamSynchronize(nullptr);
		if (he != hipSuccess) status = fail_hip(he, "nrs_envmap_create: hipStreamSynchronize");
	}
	if (status != NRS_OK) {
		nrs_envmap_destroy(e);
		return status;
	}
	*out = e;
	return NRS_OK;
}

void nrs_envmap_destroy(nrs_envmap* e) {
	if (!e) return;
	nrs_optimizer_destroy(e->opt);
	delete e; // (its buffers go with it)
}

int nrs_envmap_resolution(const nrs_envmap* e, uint32_t* res_x, uint32_t* res_y) {
	if (!e) return fail(NRS_ERR_INVALID_ARG, "nrs_envmap_resolution: NULL envmap");
	if (res_x) *res_x = e->res_x;
	if (res_y) *res_y = e->res_y;
	return NRS_OK;
}

int nrs_envmap_set_texels(nrs_envmap* e, const float* texels, int on_device, void* stream) {
	if (!e || !texels) return fail(NRS_ERR_INVALID_ARG, "nrs_envmap_set_texels: NULL argument");
	HIP_TRY(hipSetDevice(e->ctx->device));
	NRS_TRY(nrs_optimizer_set_weights(e->opt, texels, on_device, stream));
	HIP_TRY(hipMemsetAsync(e->d_grad.get(), 0, (size_t)e->n * sizeof(float), (hipStream_t)stream));
	HIP_TRY(hipMemsetAsync(e->d_cells.get(), 0, (size_t)e->n * sizeof(unsigned long long), (hipStream_t)stream));
	return NRS_OK;
}

int nrs_envmap_get(nrs_envmap* e, int which, void* h_out, size_t n) {
	if (which < NRS_ENVMAP_TEXELS || which > NRS_ENVMAP_CELLS) return fail(NRS_ERR_INVALID_ARG, "nrs_envmap_get: unknown `which`");
	if (!e || !h_out) return fail(NRS_ERR_INVALID_ARG, "nrs_envmap_get: NULL argument");
	if (n != e->n) return fail(NRS_ERR_INVALID_ARG, "nrs_envmap_get: n is not 4 * res_x * res_y");
	if (which == NRS_ENVMAP_TEXELS) return nrs_optimizer_get_state(e->opt, NRS_OPT_MASTER, h_out, n);
	if (which == NRS_ENVMAP_EMA) return nrs_optimizer_get_state(e->opt, NRS_OPT_EMA, h_out, n);
	HIP_TRY(hipSetDevice(e->ctx->device));
	HIP_TRY(hipDeviceSynchronize());
	return signed_cells_to_host(e, n, which == NRS_ENVMAP_GRADIENT, h_out); // the cells, or the gradient the next step will read (after a step: zero)
}

int nrs_envmap_export(nrs_envmap* e, int ema, float* d_out, void* stream) {
	if (!e || !d_out) return fail(NRS_ERR_INVALID_ARG, "nrs_envmap_export: NULL argument");
	HIP_TRY(hipSetDevice(e->ctx->device));
	const float* src = ema ? e->opt->d_ema.get() : e->opt->d_master.get();
	HIP_TRY(hipMemcpyAsync(d_out, src, (size_t)e->n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
	return NRS_OK;
}

int nrs_envmap_background(nrs_envmap* e, void* stream, uint32_t n_rays, const uint32_t* d_ray_counter, const uint32_t* d_ray_indices, const float* d_rays,
                          const float* d_background, const float* default_background, float* d_background_linear, int32_t* d_footprint) {
	if (!e || (n_rays && (!d_ray_counter || !d_ray_indices || !d_rays || !d_background_linear || !d_footprint)))
		return fail(NRS_ERR_INVALID_ARG, "nrs_envmap_background: NULL argument");
	if (!d_background && !default_background) return fail(NRS_ERR_INVALID_ARG, "nrs_envmap_background: neither d_background nor default_background");
	NRS_TRY(check_ray_count(n_rays, "nrs_envmap_background"));
	if (!aligned16(d_footprint)) return fail(NRS_ERR_INVALID_ARG, "nrs_envmap_background: d_footprint is not 16-byte aligned");
	if (n_rays == 0) return NRS_OK;
	HIP_TRY(hipSetDevice(e->ctx->device));
	EnvmapBackgroundArgs a{};
	a.n_rays = n_rays; a.ray_counter = d_ray_counter; a.ray_indices = d_ray_indices; a.rays = d_rays; a.background = d_background;
	for (int c = 0; c < 3; ++c) a.default_background[c] = default_background ? default_background[c] : 0.0f;
	a.texels = e->opt->d_master.get();
	a.res[0] = (int32_t)e->res_x; a.res[1] = (int32_t)e->res_y;
	a.background_linear = d_background_linear; a.footprint = d_footprint;
	NRS_LAUNCH(launch_envmap_background(a, stream));
	return NRS_OK;
}

int nrs_envmap_accumulate(nrs_envmap* e, void* stream, const nrs_envmap_accumulate_params* p, uint32_t n_rays, const uint32_t* d_ray_counter, const uint32_t* d_numsteps_out,
                          const uint32_t* d_ray_aux, const float* d_background_linear, const int32_t* d_footprint) {
	if (!e || !p || (n_rays && (!d_ray_counter || !d_numsteps_out || !d_ray_aux || !d_background_linear || !d_footprint)))
		return fail(NRS_ERR_INVALID_ARG, "nrs_envmap_accumulate: NULL argument");
	if (p->struct_size != sizeof(nrs_envmap_accumulate_params))
		return fail(NRS_ERR_INVALID_ARG, "nrs_envmap_accumulate: params->struct_size is not sizeof(nrs_envmap_accumulate_params)");
	if (p->loss_type > (uint32_t)NRS_LOSS_RELATIVE_L2 || p->envmap_loss_type > (uint32_t)NRS_LOSS_RELATIVE_L2)
		return fail(NRS_ERR_INVALID_ARG, "nrs_envmap_accumulate: unknown loss_type or envmap_loss_type");
	if (!std::isfinite(p->loss_scale)) return fail(NRS_ERR_INVALID_ARG, "nrs_envmap_accumulate: loss_scale is not finite");
	NRS_TRY(check_ray_count(n_rays, "nrs_envmap_accumulate"));
	if (!aligned16(d_ray_aux) || !aligned16(d_footprint)) return fail(NRS_ERR_INVALID_ARG, "nrs_envmap_accumulate: d_ray_aux or d_footprint is not 16-byte aligned");
	if (n_rays == 0) return NRS_OK;
	HIP_TRY(hipSetDevice(e->ctx->device));
	EnvmapAccumulateArgs a{};
	a.n_rays = n_rays; a.ray_counter = d_ray_counter; a.numsteps_out = d_numsteps_out; a.ray_aux = d_ray_aux; a.background_linear = d_background_linear;
	a.footprint = d_footprint;
	a.loss_type = p->loss_type; a.envmap_loss_type = p->envmap_loss_type; a.train_in_linear_colors = p->train_in_linear_colors ? 1u : 0u; a.loss_scale = p->loss_scale;
	a.res[0] = (int32_t)e->res_x; a.res[1] = (int32_t)e->res_y;
	a.cells = e->d_cells.get();
	NRS_LAUNCH(launch_envmap_accumulate(a, stream));
	return NRS_OK;
}

int nrs_envmap_step(nrs_envmap* e, void* stream, float loss_scale, float learning_rate) {
	if (!e) return fail(NRS_ERR_INVALID_ARG, "nrs_envmap_step: NULL envmap");
	NRS_TRY(check_step_scalars(loss_scale, learning_rate, "nrs_envmap_step"));
	HIP_TRY(hipSetDevice(e->ctx->device));
	NRS_LAUNCH(launch_envmap_cells_to_gradient(e->n, e->d_cells.get(), e->d_grad.get(), stream));
	return nrs_optimizer_step(e->opt, stream, e->d_grad.get(), loss_scale, learning_rate, 1);
}

uint32_t nrs_envmap_step_count(const nrs_envmap* e) { return e ? nrs_optimizer_step_count(e->opt) : 0u; }

} // extern "C"
