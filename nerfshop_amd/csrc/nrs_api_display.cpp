// nrs_api_display.cpp -- after the render call: accumulate, tonemap, de-tile.
#include "nrs_host.h"
#include "nrs_display.h"

#include <cmath>
#include <cstdio>

using namespace nrs;

extern "C" {

int nrs_accumulate_spp(nrs_ctx* ctx, void* stream, uint32_t width, uint32_t height, const float* d_frames, size_t slab_stride_pixels, uint32_t spp_count, float* d_accumulate,
                       uint32_t sample_count, uint32_t color_space) {
	if (!ctx || !d_frames || !d_accumulate) return fail(NRS_ERR_INVALID_ARG, "nrs_accumulate_spp: NULL argument (ctx, d_frames, d_accumulate)");
	if (color_space > NRS_COLOR_VISPOSNEG) return fail(NRS_ERR_INVALID_ARG, "nrs_accumulate_spp: color_space is 0 (Linear), 1 (SRGB) or 2 (VisPosNeg)");
	if ((uint64_t)width * height > 0xffffffffull) return fail(NRS_ERR_INVALID_ARG, "nrs_accumulate_spp: image too large");
	if (spp_count == 0u) return fail(NRS_ERR_INVALID_ARG, "nrs_accumulate_spp: spp_count is 0");
	if (spp_count > NRS_SPP_BATCH_MAX) return fail(NRS_ERR_INVALID_ARG, "nrs_accumulate_spp: spp_count above NRS_SPP_BATCH_MAX (64)");
	if ((uint64_t)slab_stride_pixels < (uint64_t)width * height) return fail(NRS_ERR_INVALID_ARG, "nrs_accumulate_spp: slab_stride_pixels is smaller than width * height");
	HIP_TRY(hipSetDevice(ctx->device));
	NRS_LAUNCH(launch_accumulate_spp(width * height, d_frames, slab_stride_pixels, spp_count, d_accumulate, sample_count, (int)color_space, stream));
	return NRS_OK;
}

int nrs_accumulate(nrs_ctx* ctx, void* stream, uint32_t width, uint32_t height, const float* d_frame, float* d_accumulate, uint32_t sample_count, uint32_t color_space) {
	if (!ctx || !d_frame || !d_accumulate) return fail(NRS_ERR_INVALID_ARG, "nrs_accumulate: NULL argument");
	if (color_space > NRS_COLOR_VISPOSNEG) return fail(NRS_ERR_INVALID_ARG, "nrs_accumulate: color_space is 0 (Linear), 1 (SRGB) or 2 (VisPosNeg)");
	if ((uint64_t)width * height > 0xffffffffull) return fail(NRS_ERR_INVALID_ARG, "nrs_accumulate: image too large");
	HIP_TRY(hipSetDevice(ctx->device));
	NRS_LAUNCH(launch_accumulate(width * height, d_frame, d_accumulate, sample_count, (int)color_space, stream));
	return NRS_OK;
}

// what nrs_tonemap and nrs_accumulate_spp_tonemap refuse in their params, before a device is touched
static int check_tonemap_params(const nrs_tonemap_params* t, uint32_t width, uint32_t height, const char* fn) {
	char msg[160];
	const char* what = nullptr;
	if (t->struct_size < sizeof(nrs_tonemap_params)) what = "params->struct_size is smaller than sizeof(nrs_tonemap_params)";
	else if (width == 0u || height == 0u) what = "width / height is 0";
	else if ((uint64_t)width * height > 0xffffffffull) what = "image too large (width * height)";
	else if (t->color_space > NRS_COLOR_VISPOSNEG) what = "params->color_space is 0 (Linear), 1 (SRGB) or 2 (VisPosNeg)";
	else if (t->output_color_space > NRS_COLOR_SRGB) what = "params->output_color_space is 0 (Linear) or 1 (SRGB)";
	else if (t->tonemap_curve > NRS_TONEMAP_REINHARD) what = "params->tonemap_curve is 0 (Identity), 1 (ACES), 2 (Hable) or 3 (Reinhard)";
	else if (t->clamp_output > 1u) what = "params->clamp_output is 0 or 1";
	else if (t->output_format != NRS_TONEMAP_RGBA32F && t->output_format != NRS_TONEMAP_RGBA8) what = "params->output_format is NRS_TONEMAP_RGBA32F or NRS_TONEMAP_RGBA8";
	else if (!std::isfinite(t->exposure)) what = "params->exposure is not finite";
	if (!what) return NRS_OK;
	snprintf(msg, sizeof(msg), "%s: %s", fn, what);
	return fail(NRS_ERR_INVALID_ARG, msg);
}

// CudaRenderBuffer::tonemap (src/render_buffer.cu:562-580)
int nrs_tonemap(nrs_ctx* ctx, void* stream, uint32_t width, uint32_t height, const float* d_accumulate, const nrs_tonemap_params* params, void* d_out) {
	if (!ctx) return fail(NRS_ERR_INVALID_ARG, "nrs_tonemap: ctx is NULL");
	if (!d_accumulate) return fail(NRS_ERR_INVALID_ARG, "nrs_tonemap: d_accumulate is NULL");
	if (!params) return fail(NRS_ERR_INVALID_ARG, "nrs_tonemap: params is NULL");
	if (!d_out) return fail(NRS_ERR_INVALID_ARG, "nrs_tonemap: d_out is NULL");
	NRS_TRY(check_tonemap_params(params, width, height, "nrs_tonemap"));
	if (params->output_format == NRS_TONEMAP_RGBA8 && d_out == (const void*)d_accumulate)
		return fail(NRS_ERR_INVALID_ARG, "nrs_tonemap: d_out is d_accumulate with NRS_TONEMAP_RGBA8 (in place is for NRS_TONEMAP_RGBA32F)");
	HIP_TRY(hipSetDevice(ctx->device));
	NRS_LAUNCH(launch_tonemap(width * height, d_accumulate, *params, d_out, stream));
	return NRS_OK;
}

// the last nrs_accumulate_spp of a view and its nrs_tonemap in one pass (render_to_cpu's tail, src/python_api.cu:160-175 -> src/testbed.cu:2761-2762)
int nrs_accumulate_spp_tonemap(nrs_ctx* ctx, void* stream, uint32_t width, uint32_t height, const float* d_frames, size_t slab_stride_pixels, uint32_t spp_count,
                               float* d_accumulate, uint32_t sample_count, const nrs_tonemap_params* params, void* d_out) {
	if (!ctx) return fail(NRS_ERR_INVALID_ARG, "nrs_accumulate_spp_tonemap: ctx is NULL");
	if (!d_frames) return fail(NRS_ERR_INVALID_ARG, "nrs_accumulate_spp_tonemap: d_frames is NULL");
	if (!d_accumulate) return fail(NRS_ERR_INVALID_ARG, "nrs_accumulate_spp_tonemap: d_accumulate is NULL");
	if (!params) return fail(NRS_ERR_INVALID_ARG, "nrs_accumulate_spp_tonemap: params is NULL");
	if (!d_out) return fail(NRS_ERR_INVALID_ARG, "nrs_accumulate_spp_tonemap: d_out is NULL");
	NRS_TRY(check_tonemap_params(params, width, height, "nrs_accumulate_spp_tonemap"));
	if (spp_count == 0u) return fail(NRS_ERR_INVALID_ARG, "nrs_accumulate_spp_tonemap: spp_count is 0");
	if (spp_count > NRS_SPP_BATCH_MAX) return fail(NRS_ERR_INVALID_ARG, "nrs_accumulate_spp_tonemap: spp_count above NRS_SPP_BATCH_MAX (64)");
	if ((uint64_t)slab_stride_pixels < (uint64_t)width * height) return fail(NRS_ERR_INVALID_ARG, "nrs_accumulate_spp_tonemap: slab_stride_pixels is smaller than width * height");
	if (d_out == (const void*)d_accumulate || d_out == (const void*)d_frames) return fail(NRS_ERR_INVALID_ARG, "nrs_accumulate_spp_tonemap: d_out aliases d_accumulate / d_frames");
	HIP_TRY(hipSetDevice(ctx->device));
	NRS_LAUNCH(launch_accumulate_spp_tonemap(width * height, d_frames, slab_stride_pixels, spp_count, d_accumulate, sample_count, *params, d_out, stream));
	return NRS_OK;
}

size_t nrs_tonemap_output_bytes(uint32_t width, uint32_t height, uint32_t output_format) {
	if (output_format != NRS_TONEMAP_RGBA32F && output_format != NRS_TONEMAP_RGBA8) return 0;
	return (size_t)width * height * (output_format == NRS_TONEMAP_RGBA32F ? 16u : 4u);
}

int nrs_detile(nrs_ctx* ctx, void* stream, const nrs_render_params* p, uint32_t n_ranks, uint32_t tiles_per_rank_padded, const float* d_tiles,
               uint32_t channels, size_t rank_stride_floats, float* d_image) {
	if (!ctx || !p || !d_tiles || !d_image) return fail(NRS_ERR_INVALID_ARG, "nrs_detile: NULL argument");
	NRS_TRY(check_params_abi(p, "nrs_detile"));
	if (p->tile_size == 0 || p->tile_size % 8 || n_ranks == 0 || channels == 0) return fail(NRS_ERR_INVALID_ARG, "nrs_detile: bad tiling");
	const size_t dense = (size_t)tiles_per_rank_padded * p->tile_size * p->tile_size * channels;
	if (rank_stride_floats == 0) rank_stride_floats = dense;
	if (rank_stride_floats < dense) return fail(NRS_ERR_INVALID_ARG, "nrs_detile: rank stride smaller than one rank's tiles");
	HIP_TRY(hipSetDevice(ctx->device));
	NRS_LAUNCH(launch_detile(*p, n_ranks, rank_stride_floats, d_tiles, channels, d_image, stream));
	return NRS_OK;
}

} // extern "C"
