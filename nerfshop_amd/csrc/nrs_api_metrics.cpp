// nrs_api_metrics.cpp -- image metrics behind the C-ABI (include/nrs.h, "image metrics"): the device call on a caller's reference and on a dataset image, the CPU twin
// and run.py's totals.  Everything that can be refused is refused before the first HIP call.
#include "nrs_handles.h"
#include "nrs_metrics.h"

#include <cmath>
#include <limits>

using namespace nrs;

// what all three calls refuse in their sizes and params; `px` receives what the kernel and the twin read of them
static int check_metrics_args(uint32_t width, uint32_t height, const nrs_image_metrics_params* p, MetricsPixelArgs* px, const char* fn) {
	const std::string who(fn);
	if (p->struct_size != sizeof(nrs_image_metrics_params)) return fail(NRS_ERR_INVALID_ARG, who + ": params->struct_size is not sizeof(nrs_image_metrics_params)");
	if (width == 0 || height == 0) return fail(NRS_ERR_INVALID_ARG, who + ": width or height is 0");
	if (width > NRS_IMAGE_METRICS_MAX_DIM || height > NRS_IMAGE_METRICS_MAX_DIM) return fail(NRS_ERR_INVALID_ARG, who + ": width or height above 8192 (what the 64-bit sums hold)");
	if (p->reference_format != NRS_IMAGE_RGBA16F_LINEAR && p->reference_format != NRS_IMAGE_RGBA32F_LINEAR)
		return fail(NRS_ERR_INVALID_ARG, who + ": params->reference_format is NRS_IMAGE_RGBA16F_LINEAR or NRS_IMAGE_RGBA32F_LINEAR");
	for (int c = 0; c < 4; ++c)
		if (!std::isfinite(p->background_color[c])) return fail(NRS_ERR_INVALID_ARG, who + ": params->background_color is not finite");
	px->srgb_blend = p->color_space == NRS_COLOR_SRGB ? 1 : 0;
	for (int c = 0; c < 3; ++c) px->bg[c] = p->background_color[c];
	return NRS_OK;
}
static bool aligned(const void* p, uintptr_t a) { return p == nullptr || ((uintptr_t)p & (a - 1)) == 0; }
static int check_device_pointers(const float* d_image, const void* d_reference, uint32_t reference_format, const void* d_result, const float* d_ssim_map, const float* d_sq_err_map,
                                 const char* fn) {
	if (!aligned(d_image, 16) || !aligned(d_reference, reference_format == NRS_IMAGE_RGBA16F_LINEAR ? 8 : 16) || !aligned(d_result, 8) || !aligned(d_ssim_map, 4) ||
	    !aligned(d_sq_err_map, 4))
		return fail(NRS_ERR_INVALID_ARG, std::string(fn) + ": a misaligned pointer (d_image 16 bytes, d_reference 8 / 16, d_result 8, the maps 4)");
	return NRS_OK;
}

extern "C" {

int nrs_image_metrics(nrs_ctx* ctx, void* stream, uint32_t width, uint32_t height, const float* d_image, const void* d_reference, const nrs_image_metrics_params* params,
                      nrs_image_metrics_result* d_result, float* d_ssim_map, float* d_sq_err_map) {
	if (!ctx || !d_image || !d_reference || !params || !d_result) return fail(NRS_ERR_INVALID_ARG, "nrs_image_metrics: NULL argument (ctx, d_image, d_reference, params, d_result)");
	MetricsPixelArgs px{};
	NRS_TRY(check_metrics_args(width, height, params, &px, "nrs_image_metrics"));
	NRS_TRY(check_device_pointers(d_image, d_reference, params->reference_format, d_result, d_ssim_map, d_sq_err_map, "nrs_image_metrics"));
	HIP_TRY(hipSetDevice(ctx->device));
	NRS_LAUNCH(launch_image_metrics(width, height, d_image, d_reference, (int)params->reference_format, px, d_result, d_ssim_map, d_sq_err_map, stream));
	return NRS_OK;
}

int nrs_dataset_image_metrics(nrs_dataset* ds, uint32_t index, void* stream, const float* d_image, const nrs_image_metrics_params* params, nrs_image_metrics_result* d_result,
                              float* d_ssim_map, float* d_sq_err_map) {
	if (!ds || !d_image || !params || !d_result) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_image_metrics: NULL argument (ds, d_image, params, d_result)");
	MetricsPixelArgs px{};
	NRS_TRY(check_metrics_args(ds->width, ds->height, params, &px, "nrs_dataset_image_metrics"));
	if (params->reference_format != NRS_IMAGE_RGBA16F_LINEAR) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_image_metrics: params->reference_format is NRS_IMAGE_RGBA16F_LINEAR (what a dataset stores)");
	if (index >= ds->n_images) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_image_metrics: index past n_images");
	NRS_TRY(check_device_pointers(d_image, nullptr, params->reference_format, d_result, d_ssim_map, d_sq_err_map, "nrs_dataset_image_metrics"));
	if (!ds->image_set[index]) return fail(NRS_ERR_STATE, "nrs_dataset_image_metrics: the image has never been set (nrs_dataset_set_image)");
	HIP_TRY(hipSetDevice(ds->ctx->device));
	const uint64_t* ref = ds->d_images.get() + (size_t)index * ds->width * ds->height;
	NRS_LAUNCH(launch_image_metrics(ds->width, ds->height, d_image, ref, NRS_IMAGE_RGBA16F_LINEAR, px, d_result, d_ssim_map, d_sq_err_map, stream));
	return NRS_OK;
}

int nrs_image_metrics_host(uint32_t width, uint32_t height, const float* h_image, const void* h_reference, const nrs_image_metrics_params* params,
                           nrs_image_metrics_result* h_result, float* h_ssim_map, float* h_sq_err_map) {
	if (!h_image || !h_reference || !params || !h_result) return fail(NRS_ERR_INVALID_ARG, "nrs_image_metrics_host: NULL argument (h_image, h_reference, params, h_result)");
	MetricsPixelArgs px{};
	NRS_TRY(check_metrics_args(width, height, params, &px, "nrs_image_metrics_host"));
	image_metrics_host((int)width, (int)height, h_image, h_reference, params->reference_format == NRS_IMAGE_RGBA16F_LINEAR, px, h_result, h_ssim_map, h_sq_err_map);
	return NRS_OK;
}

// run.py:292-301
int nrs_image_metrics_summary_host(const nrs_image_metrics_result* h_results, uint32_t n, nrs_metrics_summary* out) {
	if (!h_results || !out) return fail(NRS_ERR_INVALID_ARG, "nrs_image_metrics_summary_host: NULL argument");
	if (n == 0) return fail(NRS_ERR_INVALID_ARG, "nrs_image_metrics_summary_host: n is 0");
	double tot_psnr = 0, tot_ssim = 0, tot_mse = 0;
	double mn = std::numeric_limits<double>::infinity(), mx = -std::numeric_limits<double>::infinity();
	for (uint32_t i = 0; i < n; ++i) {
		const double psnr = (double)h_results[i].psnr;
		tot_psnr += psnr;
		tot_ssim += (double)h_results[i].ssim;
		tot_mse += (double)h_results[i].mse;
		mn = psnr < mn ? psnr : mn;
		mx = psnr > mx ? psnr : mx;
	}
	const double mean_mse = tot_mse / n;
	out->psnr_mean = tot_psnr / n;
	out->psnr_min = mn;
	out->psnr_max = mx;
	out->ssim_mean = tot_ssim / n;
	out->psnr_avgmse = mean_mse == 0.0 ? std::numeric_limits<double>::infinity() : -10.0 * std::log10(mean_mse);
	out->n_views = n;
	out->reserved = 0;
	return NRS_OK;
}

} // extern "C"
