// nrs_api_train.cpp -- the training-ray path behind the C-ABI: nrs_training_samples, nrs_ray_loss, nrs_ray_loss_ex.  Everything that can be refused is refused before the first HIP call.
#include "nrs_train_host.h"
#include "nrs_train.h"

#include <cmath>

using namespace nrs;

// The model's per-ray workspace, at least `words` long: allocated on the first call of a size (hipFree of the smaller one waits for the device), reused afterwards.
static int train_workspace(nrs_model* m, size_t words, const char* who) {
	if (m->d_train_ws.count() >= words) return NRS_OK;
	const hipError_t e = m->d_train_ws.alloc(words);
	if (e != hipSuccess) return fail_hip(e, who);
	return NRS_OK;
}

extern "C" {

int nrs_training_samples(nrs_model* m, void* stream, uint32_t n_rays, const float* d_rays, const float* d_jitter, float cone_angle_constant, uint32_t max_samples,
                         float* d_coords_out, uint32_t ld, uint32_t* d_numsteps_out, uint32_t* d_ray_indices_out, uint32_t* d_counters) {
	if (!m || !d_coords_out || !d_counters || (n_rays && (!d_rays || !d_numsteps_out || !d_ray_indices_out)))
		return fail(NRS_ERR_INVALID_ARG, "nrs_training_samples: NULL argument");
	if (ld < NRS_NETWORK_INPUT_FLOATS) return fail(NRS_ERR_INVALID_ARG, "nrs_training_samples: ld < 7");
	if (max_samples == 0) return fail(NRS_ERR_INVALID_ARG, "nrs_training_samples: max_samples is 0");
	if (!(cone_angle_constant >= 0.f) || !std::isfinite(cone_angle_constant)) return fail(NRS_ERR_INVALID_ARG, "nrs_training_samples: cone_angle_constant is negative or not finite");
	NRS_TRY(check_ray_count(n_rays, "nrs_training_samples", " (the sample counters are 32 bits wide)"));
	if (m->n_extra_dims != 0u) return fail(NRS_ERR_UNSUPPORTED, "nrs_training_samples: n_extra_dims (0 is supported: no training samples with light directions)");
	if (!m->have_bitfield) return fail(NRS_ERR_STATE, "nrs_training_samples: occupancy not set (nrs_model_set_density_bitfield/_grid)");
	HIP_TRY(hipSetDevice(m->ctx->device));
	if (n_rays) NRS_TRY(train_workspace(m, train_ws_words<TrainSamplesWs>(n_rays), "nrs_training_samples: workspace allocation"));
	TrainSamplesArgs a{};
	a.n_rays = n_rays; a.rays = d_rays; a.jitter = d_jitter; a.cone = cone_angle_constant; a.max_samples = max_samples;
	a.coords = d_coords_out; a.ld = ld; a.numsteps = d_numsteps_out; a.ray_indices = d_ray_indices_out; a.counters = d_counters;
	a.ws = n_rays ? m->d_train_ws.get() : nullptr;
	NRS_LAUNCH(launch_training_samples(m->dm, a, stream));
	return NRS_OK;
}

int nrs_ray_loss(nrs_model* m, void* stream, const nrs_ray_loss_params* p, uint32_t n_rays, const uint32_t* d_ray_counter, const uint32_t* d_numsteps, uint32_t n_samples,
                 const float* d_coords, uint32_t ld_in, const void* d_output_fp16, uint32_t ld_out, int out_layout, const float* d_target_rgba, const float* d_background,
                 const float* d_ray_origins, uint32_t* d_numsteps_out, float* d_coords_out, void* d_dL_doutput_fp16, uint32_t ld_dl, int dl_layout, float* d_loss,
                 uint32_t* d_counter_out) {
	return nrs_ray_loss_ex(m, stream, p, n_rays, d_ray_counter, d_numsteps, n_samples, d_coords, ld_in, d_output_fp16, ld_out, out_layout, d_target_rgba, d_background,
	                       d_ray_origins, d_numsteps_out, d_coords_out, d_dL_doutput_fp16, ld_dl, dl_layout, d_loss, d_counter_out, nullptr, nullptr);
}

// (the messages name nrs_ray_loss for both doors: one body)
int nrs_ray_loss_ex(nrs_model* m, void* stream, const nrs_ray_loss_params* p, uint32_t n_rays, const uint32_t* d_ray_counter, const uint32_t* d_numsteps, uint32_t n_samples,
                    const float* d_coords, uint32_t ld_in, const void* d_output_fp16, uint32_t ld_out, int out_layout, const float* d_target_rgba, const float* d_background,
                    const float* d_ray_origins, uint32_t* d_numsteps_out, float* d_coords_out, void* d_dL_doutput_fp16, uint32_t ld_dl, int dl_layout, float* d_loss,
                    uint32_t* d_counter_out, const float* d_background_linear, uint32_t* d_ray_aux) {
	if (!m || !p || !d_coords_out || !d_dL_doutput_fp16 || !d_counter_out || (n_rays && (!d_numsteps || !d_coords || !d_output_fp16 || !d_target_rgba || !d_numsteps_out)))
		return fail(NRS_ERR_INVALID_ARG, "nrs_ray_loss: NULL argument");
	if (p->struct_size != sizeof(nrs_ray_loss_params)) return fail(NRS_ERR_INVALID_ARG, "nrs_ray_loss: params->struct_size is not sizeof(nrs_ray_loss_params)");
	if (n_rays && d_numsteps_out == d_numsteps) return fail(NRS_ERR_INVALID_ARG, "nrs_ray_loss: d_numsteps_out aliases d_numsteps");
	if (p->loss_type > (uint32_t)NRS_LOSS_RELATIVE_L2) return fail(NRS_ERR_INVALID_ARG, "nrs_ray_loss: unknown loss_type");
	if (p->color_space != (uint32_t)NRS_COLOR_LINEAR && p->color_space != (uint32_t)NRS_COLOR_SRGB)
		return fail(NRS_ERR_INVALID_ARG, "nrs_ray_loss: color_space is neither NRS_COLOR_LINEAR nor NRS_COLOR_SRGB");
	if ((out_layout != NRS_PLANES && out_layout != NRS_INTERLEAVED) || (dl_layout != NRS_PLANES && dl_layout != NRS_INTERLEAVED))
		return fail(NRS_ERR_INVALID_ARG, "nrs_ray_loss: layout is neither NRS_PLANES nor NRS_INTERLEAVED");
	if (ld_in < NRS_NETWORK_INPUT_FLOATS) return fail(NRS_ERR_INVALID_ARG, "nrs_ray_loss: ld_in < 7");
	if (p->max_samples_compacted == 0) return fail(NRS_ERR_INVALID_ARG, "nrs_ray_loss: max_samples_compacted is 0");
	if (out_layout == NRS_PLANES && ld_out < n_samples) return fail(NRS_ERR_INVALID_ARG, "nrs_ray_loss: ld_out < n_samples");
	if (dl_layout == NRS_PLANES && ld_dl < p->max_samples_compacted) return fail(NRS_ERR_INVALID_ARG, "nrs_ray_loss: ld_dl < max_samples_compacted");
	if (!std::isfinite(p->loss_scale)) return fail(NRS_ERR_INVALID_ARG, "nrs_ray_loss: loss_scale is not finite");
	if (p->near_distance > 0.f && !d_ray_origins) return fail(NRS_ERR_INVALID_ARG, "nrs_ray_loss: near_distance > 0 needs d_ray_origins");
	NRS_TRY(check_ray_count(n_rays, "nrs_ray_loss", " (the sample counters are 32 bits wide)"));
	if (!aligned16(d_ray_aux)) return fail(NRS_ERR_INVALID_ARG, "nrs_ray_loss_ex: d_ray_aux is not 16-byte aligned");
	if (n_rays) { // the compaction is not done in place
		const char *in0 = (const char*)d_coords, *in1 = in0 + (size_t)n_samples * ld_in * sizeof(float);
		const char *out0 = (const char*)d_coords_out, *out1 = out0 + (size_t)p->max_samples_compacted * ld_in * sizeof(float);
		if (in0 < out1 && out0 < in1) return fail(NRS_ERR_INVALID_ARG, "nrs_ray_loss: d_coords_out overlaps d_coords");
	}
	HIP_TRY(hipSetDevice(m->ctx->device));
	if (n_rays) NRS_TRY(train_workspace(m, train_ws_words<RayLossWs>(n_rays), "nrs_ray_loss: workspace allocation"));
	RayLossArgs a{};
	a.p = *p; a.n_rays = n_rays; a.ray_counter = d_ray_counter; a.numsteps = d_numsteps; a.n_samples = n_samples; a.coords = d_coords; a.ld_in = ld_in;
	a.output = d_output_fp16; a.ld_out = ld_out; a.out_layout = out_layout; a.target_rgba = d_target_rgba; a.background = d_background; a.origins = d_ray_origins;
	a.numsteps_out = d_numsteps_out; a.coords_out = d_coords_out; a.dl = d_dL_doutput_fp16; a.ld_dl = ld_dl; a.dl_layout = dl_layout; a.loss = d_loss;
	a.counter_out = d_counter_out; a.background_linear = d_background_linear; a.ray_aux = d_ray_aux;
	a.ws = n_rays ? m->d_train_ws.get() : nullptr;
	NRS_LAUNCH(launch_ray_loss(m->dm, a, stream));
	return NRS_OK;
}

} // extern "C"
