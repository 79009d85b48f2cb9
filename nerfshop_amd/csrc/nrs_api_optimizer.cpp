// nrs_api_optimizer.cpp -- the optimiser behind the C-ABI (include/nrs.h, "optimiser"): the bias table and the schedule on the host, the handle, the step.
// Everything that can be refused is refused before the first HIP call; nrs_optimizer_step never waits for the device.
#include "nrs_train_host.h"
#include "nrs_optimizer.h"

#include <cmath>
#include <cstdlib>
#include <new>

using namespace nrs;

namespace {

double bias_f64(double b1, double b2, uint32_t t) { return std::sqrt(1.0 - std::pow(b2, (double)t)) / (1.0 - std::pow(b1, (double)t)); }

// bias(t) rounded once to fp32 for t = 1 .. T_sat at table[t - 1]; T_sat = the first t from which on the rounded value is exactly 1.0f
int make_bias_table(float beta1, float beta2, std::vector<float>& table, const char* who) {
	if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) return fail(NRS_ERR_INVALID_ARG, std::string(who) + ": beta1 / beta2 outside [0, 1)");
	const double b1 = beta1, b2 = beta2, bmax = std::max(b1, b2);
	// from t_hi on both powers are below 2^-30: the quotient is within 2^-30 of 1 and rounds to 1.0f for good
	const double t_hi_d = bmax > 0.0 ? std::ceil(-30.0 * std::log(2.0) / std::log(bmax)) + 1.0 : 1.0;
	if (t_hi_d > 2.0 * kAdamTableMax) return fail(NRS_ERR_INVALID_ARG, std::string(who) + ": the bias table would exceed 65536 entries (a beta too close to 1)");
	uint32_t t_sat = (uint32_t)t_hi_d;
	while (t_sat > 1u && (float)bias_f64(b1, b2, t_sat - 1u) == 1.0f) --t_sat;
	if (t_sat > kAdamTableMax) return fail(NRS_ERR_INVALID_ARG, std::string(who) + ": the bias table would exceed 65536 entries (a beta too close to 1)");
	table.resize(t_sat);
	for (uint32_t t = 1; t <= t_sat; ++t) table[t - 1] = (float)bias_f64(b1, b2, t);
	return NRS_OK;
}

bool finite_nonneg(float x) { return std::isfinite(x) && x >= 0.f; }

int check_adam_params(const nrs_adam_params* p, const char* who) {
	const std::string w(who);
	if (!p) return fail(NRS_ERR_INVALID_ARG, w + ": params is NULL");
	if (p->struct_size != sizeof(nrs_adam_params)) return fail(NRS_ERR_INVALID_ARG, w + ": params->struct_size is not sizeof(nrs_adam_params)");
	if (!(p->beta1 >= 0.f && p->beta1 < 1.f)) return fail(NRS_ERR_INVALID_ARG, w + ": beta1 outside [0, 1)");
	if (!(p->beta2 >= 0.f && p->beta2 < 1.f)) return fail(NRS_ERR_INVALID_ARG, w + ": beta2 outside [0, 1)");
	if (!finite_nonneg(p->epsilon)) return fail(NRS_ERR_INVALID_ARG, w + ": epsilon is negative or not finite");
	if (!finite_nonneg(p->l2_reg)) return fail(NRS_ERR_INVALID_ARG, w + ": l2_reg is negative or not finite");
	if (!finite_nonneg(p->non_matrix_lr_factor)) return fail(NRS_ERR_INVALID_ARG, w + ": non_matrix_lr_factor is negative or not finite");
	if (!(p->ema_decay >= 0.f && p->ema_decay < 1.f)) return fail(NRS_ERR_INVALID_ARG, w + ": ema_decay outside [0, 1)");
	return NRS_OK;
}

Fp16Dest fp16_dest(nrs_optimizer* o) { return Fp16Dest{o->d_fp16.get(), o->model ? model_grid_fp16(o->model) : o->d_fp16.get(), o->split}; }

// after the fp16 copy has been written on `stream`: a bound model's fragments and records follow on the same stream
int publish(nrs_optimizer* o, void* stream) {
	if (!o->model) return NRS_OK;
	NRS_TRY(model_mlp_from_device(o->model, o->d_fp16.get(), stream));
	return model_grid_written(o->model, stream);
}

// checked arguments; `model` may be NULL
int optimizer_create(nrs_ctx* ctx, nrs_model* model, size_t n, size_t n_matrix, uint32_t split, const nrs_adam_params* p, std::vector<float>& table, nrs_optimizer** out,
                     const char* who) {
	HIP_TRY(hipSetDevice(ctx->device));
	nrs_optimizer* o = new (std::nothrow) nrs_optimizer();
	if (!o) return fail(NRS_ERR_STATE, "out of host memory");
	o->ctx = ctx; o->model = model; o->p = *p;
	o->n = (uint32_t)n; o->n_matrix = (uint32_t)n_matrix; o->split = split;
	o->t_sat = (uint32_t)table.size();
	if (const char* e = getenv("NRS_OPTIMIZER_VARIANT")) o->variant = (uint32_t)atoi(e);
	table.insert(table.begin(), 0.0f); // index t
	hipError_t he = o->d_master.alloc(n);
	if (he == hipSuccess) he = o->d_m.alloc(n);
	if (he == hipSuccess) he = o->d_v.alloc(n);
	if (he == hipSuccess) he = o->d_ema.alloc(n);
	if (he == hipSuccess) he = o->d_steps.alloc(n);
	if (he == hipSuccess) he = o->d_fp16.alloc(split);
	if (he == hipSuccess) he = o->d_table.alloc(table.size());
	if (he == hipSuccess) he = hipMemcpy(o->d_table.get(), table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice);
	if (he != hipSuccess) {
		delete o;
		return fail_hip(he, (std::string(who) + ": device allocation").c_str());
	}
	*out = o;
	return NRS_OK;
}

size_t state_element_bytes(int which) { return which == NRS_OPT_PARAMS_FP16 ? 2 : 4; }
void* state_pointer(nrs_optimizer* o, int which) {
	switch (which) {
	case NRS_OPT_MASTER: return o->d_master.get();
	case NRS_OPT_M: return o->d_m.get();
	case NRS_OPT_V: return o->d_v.get();
	case NRS_OPT_STEPS: return o->d_steps.get();
	case NRS_OPT_EMA: return o->d_ema.get();
	default: return nullptr;
	}
}
int check_state_call(nrs_optimizer* o, int which, const void* h, size_t n, const char* who) {
	const std::string w(who);
	if (which < NRS_OPT_MASTER || which > NRS_OPT_PARAMS_FP16) return fail(NRS_ERR_INVALID_ARG, w + ": unknown `which`");
	if (!o || !h) return fail(NRS_ERR_INVALID_ARG, w + ": NULL argument");
	if (n != o->n) return fail(NRS_ERR_INVALID_ARG, w + ": n is not the optimiser's n_params");
	if (!o->have_weights) return fail(NRS_ERR_STATE, w + ": weights not set (nrs_optimizer_set_weights)");
	return NRS_OK;
}

} // namespace

extern "C" {

int nrs_adam_bias_table(float beta1, float beta2, float* out, uint32_t cap, uint32_t* n_out) {
	if (!n_out) return fail(NRS_ERR_INVALID_ARG, "nrs_adam_bias_table: n_out is NULL");
	std::vector<float> table;
	NRS_TRY(make_bias_table(beta1, beta2, table, "nrs_adam_bias_table"));
	*n_out = (uint32_t)table.size();
	if (!out) return NRS_OK;
	if (cap < table.size()) return fail(NRS_ERR_INVALID_ARG, "nrs_adam_bias_table: cap is smaller than the table");
	std::copy(table.begin(), table.end(), out);
	return NRS_OK;
}

float nrs_exponential_decay_lr(float base, uint32_t decay_start, uint32_t decay_interval, float decay_base, uint32_t steps_done) {
	const uint32_t k = steps_done < decay_start ? 0u : (steps_done - decay_start) / std::max(decay_interval, 1u) + 1u;
	return (float)((double)base * std::pow((double)decay_base, (double)k));
}

int nrs_optimizer_create(nrs_ctx* ctx, size_t n_params, size_t n_matrix, const nrs_adam_params* params, nrs_optimizer** out) {
	NRS_TRY(check_adam_params(params, "nrs_optimizer_create"));
	std::vector<float> table;
	NRS_TRY(make_bias_table(params->beta1, params->beta2, table, "nrs_optimizer_create"));
	if (n_params == 0 || n_params > kAdamMaxParams) return fail(NRS_ERR_INVALID_ARG, "nrs_optimizer_create: n_params is 0 or more than 2^31");
	if (n_matrix > n_params) return fail(NRS_ERR_INVALID_ARG, "nrs_optimizer_create: n_matrix > n_params");
	if (!ctx || !out) return fail(NRS_ERR_INVALID_ARG, "nrs_optimizer_create: NULL argument");
	return optimizer_create(ctx, nullptr, n_params, n_matrix, (uint32_t)n_params, params, table, out, "nrs_optimizer_create");
}

int nrs_optimizer_create_for_model(nrs_model* model, const nrs_adam_params* params, nrs_optimizer** out) {
	NRS_TRY(check_adam_params(params, "nrs_optimizer_create_for_model"));
	std::vector<float> table;
	NRS_TRY(make_bias_table(params->beta1, params->beta2, table, "nrs_optimizer_create_for_model"));
	if (!model || !out) return fail(NRS_ERR_INVALID_ARG, "nrs_optimizer_create_for_model: NULL argument");
	if (model->n_extra_dims != 0u) return fail(NRS_ERR_UNSUPPORTED, "nrs_optimizer_create_for_model: n_extra_dims (0 is supported: no training with light directions)");
	uint32_t n_mlp = 0;
	size_t n = 0;
	model_param_counts(model, &n_mlp, &n);
	if (n == 0 || n > kAdamMaxParams) return fail(NRS_ERR_INVALID_ARG, "nrs_optimizer_create_for_model: the model has no parameters or more than 2^31");
	return optimizer_create(model->ctx, model, n, n_mlp, n_mlp, params, table, out, "nrs_optimizer_create_for_model");
}

void nrs_optimizer_destroy(nrs_optimizer* opt) {
	delete opt; // (its buffers go with it)
}

int nrs_optimizer_set_weights(nrs_optimizer* o, const float* weights, int on_device, void* stream) {
	if (!o || !weights) return fail(NRS_ERR_INVALID_ARG, "nrs_optimizer_set_weights: NULL argument");
	HIP_TRY(hipSetDevice(o->ctx->device));
	const hipStream_t s = (hipStream_t)stream;
	const size_t bytes = (size_t)o->n * 4;
	HIP_TRY(hipMemcpyAsync(o->d_master.get(), weights, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
	if (!on_device) HIP_TRY(hipStreamSynchronize(s)); // the caller's array is free again when this returns
	HIP_TRY(hipMemsetAsync(o->d_m.get(), 0, bytes, s));
	HIP_TRY(hipMemsetAsync(o->d_v.get(), 0, bytes, s));
	HIP_TRY(hipMemsetAsync(o->d_steps.get(), 0, bytes, s));
	NRS_LAUNCH(launch_adam_init(o->n, o->d_master.get(), o->d_ema.get(), fp16_dest(o), stream));
	o->step_count = 0;
	o->have_weights = true;
	return publish(o, stream);
}

int nrs_optimizer_step(nrs_optimizer* o, void* stream, float* d_grad, float loss_scale, float learning_rate, int zero_grad) {
	if (!o || !d_grad) return fail(NRS_ERR_INVALID_ARG, "nrs_optimizer_step: NULL argument");
	NRS_TRY(check_step_scalars(loss_scale, learning_rate, "nrs_optimizer_step"));
	if (((uintptr_t)d_grad & 3u) != 0u) return fail(NRS_ERR_INVALID_ARG, "nrs_optimizer_step: d_grad is not 4-byte aligned");
	if (!o->have_weights) return fail(NRS_ERR_STATE, "nrs_optimizer_step: weights not set (nrs_optimizer_set_weights)");
	HIP_TRY(hipSetDevice(o->ctx->device));
	const uint32_t T = o->step_count + 1u;
	AdamStepArgs a{};
	a.n = o->n; a.n_matrix = o->n_matrix;
	a.grad = d_grad; a.master = o->d_master.get(); a.m = o->d_m.get(); a.v = o->d_v.get(); a.steps = o->d_steps.get(); a.ema = o->d_ema.get();
	a.h = fp16_dest(o);
	a.table = o->d_table.get(); a.t_sat = o->t_sat;
	a.loss_scale = loss_scale; a.beta1 = o->p.beta1; a.beta2 = o->p.beta2;
	a.one_minus_beta1 = 1.0f - o->p.beta1; a.one_minus_beta2 = 1.0f - o->p.beta2;
	a.epsilon = o->p.epsilon; a.l2_reg = o->p.l2_reg;
	a.lr_matrix = learning_rate * 1.0f; a.lr_other = learning_rate * o->p.non_matrix_lr_factor;
	a.ema_on = o->p.ema_decay > 0.f ? 1u : 0u;
	if (a.ema_on) {
		const double d = o->p.ema_decay, den = 1.0 - std::pow(d, (double)T);
		a.ema_a = (float)(d * (1.0 - std::pow(d, (double)(T - 1u))) / den);
		a.ema_b = (float)((1.0 - d) / den);
	}
	a.zero_grad = zero_grad ? 1u : 0u;
	a.variant = o->variant;
	NRS_LAUNCH(launch_adam_step(a, stream));
	o->step_count = T;
	return publish(o, stream);
}

int nrs_optimizer_get_state(nrs_optimizer* o, int which, void* h_out, size_t n) {
	NRS_TRY(check_state_call(o, which, h_out, n, "nrs_optimizer_get_state"));
	HIP_TRY(hipSetDevice(o->ctx->device));
	HIP_TRY(hipDeviceSynchronize());
	if (which != NRS_OPT_PARAMS_FP16) {
		HIP_TRY(hipMemcpy(h_out, state_pointer(o, which), n * state_element_bytes(which), hipMemcpyDeviceToHost));
		return NRS_OK;
	}
	const Fp16Dest h = fp16_dest(o);
	HIP_TRY(hipMemcpy(h_out, h.h_lo, (size_t)h.split * 2, hipMemcpyDeviceToHost));
	if (o->n > h.split) HIP_TRY(hipMemcpy((uint16_t*)h_out + h.split, h.h_hi, (size_t)(o->n - h.split) * 2, hipMemcpyDeviceToHost));
	return NRS_OK;
}

int nrs_optimizer_set_state(nrs_optimizer* o, int which, const void* h_in, size_t n) {
	NRS_TRY(check_state_call(o, which, h_in, n, "nrs_optimizer_set_state"));
	HIP_TRY(hipSetDevice(o->ctx->device));
	HIP_TRY(hipDeviceSynchronize());
	if (which != NRS_OPT_PARAMS_FP16) {
		HIP_TRY(hipMemcpy(state_pointer(o, which), h_in, n * state_element_bytes(which), hipMemcpyHostToDevice));
		return NRS_OK;
	}
	const Fp16Dest h = fp16_dest(o);
	HIP_TRY(hipMemcpy(h.h_lo, h_in, (size_t)h.split * 2, hipMemcpyHostToDevice));
	if (o->n > h.split) HIP_TRY(hipMemcpy(h.h_hi, (const uint16_t*)h_in + h.split, (size_t)(o->n - h.split) * 2, hipMemcpyHostToDevice));
	NRS_TRY(publish(o, nullptr));
	HIP_TRY(hipStreamSynchronize(nullptr));
	return NRS_OK;
}

int nrs_optimizer_export_fp16(nrs_optimizer* o, int which, void* d_out, void* stream) {
	if (which != NRS_OPT_EXPORT_WEIGHTS && which != NRS_OPT_EXPORT_EMA) return fail(NRS_ERR_INVALID_ARG, "nrs_optimizer_export_fp16: unknown `which`");
	if (!o || !d_out) return fail(NRS_ERR_INVALID_ARG, "nrs_optimizer_export_fp16: NULL argument");
	if (!o->have_weights) return fail(NRS_ERR_STATE, "nrs_optimizer_export_fp16: weights not set (nrs_optimizer_set_weights)");
	HIP_TRY(hipSetDevice(o->ctx->device));
	const hipStream_t s = (hipStream_t)stream;
	if (which == NRS_OPT_EXPORT_EMA) {
		NRS_LAUNCH(launch_round_fp16(o->n, o->d_ema.get(), (uint16_t*)d_out, stream));
		return NRS_OK;
	}
	const Fp16Dest h = fp16_dest(o);
	HIP_TRY(hipMemcpyAsync(d_out, h.h_lo, (size_t)h.split * 2, hipMemcpyDeviceToDevice, s));
	if (o->n > h.split) HIP_TRY(hipMemcpyAsync((uint16_t*)d_out + h.split, h.h_hi, (size_t)(o->n - h.split) * 2, hipMemcpyDeviceToDevice, s));
	return NRS_OK;
}

uint32_t nrs_optimizer_step_count(const nrs_optimizer* o) { return o ? o->step_count : 0u; }

int nrs_optimizer_set_step_count(nrs_optimizer* o, uint32_t steps) {
	if (!o) return fail(NRS_ERR_INVALID_ARG, "nrs_optimizer_set_step_count: NULL optimiser");
	o->step_count = steps;
	return NRS_OK;
}

size_t nrs_optimizer_n_params(const nrs_optimizer* o, size_t* n_matrix) {
	if (!o) return 0;
	if (n_matrix) *n_matrix = o->n_matrix;
	return o->n;
}

} // extern "C"
