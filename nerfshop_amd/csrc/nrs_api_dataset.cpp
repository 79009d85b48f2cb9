// nrs_api_dataset.cpp -- the dataset behind the C-ABI: create / destroy, images (converted on the device), cameras (kept on the host, sent in one block), the pixel
// rays of a training step, mark_untrained, and the training error map (its cells, its CDFs, the rays drawn from them).  Everything that can be refused is refused before the first HIP call.
#include "nrs_train_host.h"
#include "nrs_dataset.h"
#include "nrs_train.h"
#include "nrs_cells.h"

#include <cmath>
#include <cstring>
#include <new>

using namespace nrs;

// the camera block on the device, as the host holds it (the call waits for the copy: the next nrs_dataset_set_camera may rewrite the host's records at once)
static int send_cameras(nrs_dataset* ds, hipStream_t s) {
	if (!ds->cameras_dirty) return NRS_OK;
	HIP_TRY(hipMemcpyAsync(ds->d_cameras.get(), ds->cameras.data(), ds->cameras.size() * sizeof(float), hipMemcpyHostToDevice, s));
	HIP_TRY(hipStreamSynchronize(s));
	ds->cameras_dirty = false;
	return NRS_OK;
}
static int check_complete(const nrs_dataset* ds, const char* who) {
	if (ds->n_images_set != ds->n_images) return fail(NRS_ERR_STATE, std::string(who) + ": an image has never been set (nrs_dataset_set_image)");
	if (ds->n_cameras_set != ds->n_images) return fail(NRS_ERR_STATE, std::string(who) + ": a camera has never been set (nrs_dataset_set_camera)");
	return NRS_OK;
}

extern "C" {

int nrs_dataset_create(nrs_ctx* ctx, uint32_t n_images, uint32_t width, uint32_t height, nrs_dataset** out) {
	if (!ctx || !out) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_create: NULL argument");
	if (n_images == 0) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_create: n_images is 0");
	if (width == 0 || height == 0) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_create: width or height is 0");
	if ((uint64_t)width * height > 0x7fffffffull) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_create: width x height does not fit 31 bits (the pixel index is a 32-bit word)");
	nrs_dataset* ds = new (std::nothrow) nrs_dataset();
	if (!ds) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_create: out of host memory");
	ds->ctx = ctx; ds->n_images = n_images; ds->width = width; ds->height = height;
	ds->cameras.assign((size_t)n_images * kCameraWords, 0.f);
	ds->image_set.assign(n_images, 0);
	ds->camera_set.assign(n_images, 0);
	hipError_t e = hipSetDevice(ctx->device);
	if (e == hipSuccess) e = ds->d_images.alloc((size_t)n_images * width * height);
	if (e == hipSuccess) e = ds->d_cameras.alloc((size_t)n_images * kCameraWords);
	if (e != hipSuccess) {
		delete ds;
		return fail_hip(e, "nrs_dataset_create: allocation");
	}
	*out = ds;
	return NRS_OK;
}

void nrs_dataset_destroy(nrs_dataset* ds) {
	if (!ds) return;
	(void)hipSetDevice(ds->ctx->device);
	delete ds;
}

int nrs_dataset_set_image(nrs_dataset* ds, uint32_t index, int format, const void* pixels, int is_device_pointer, uint32_t flags, uint32_t mask_color, void* stream) {
	if (!ds || !pixels) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_set_image: NULL argument");
	if (format != NRS_IMAGE_RGBA8_SRGB && format != NRS_IMAGE_RGBA32F_LINEAR && format != NRS_IMAGE_RGBA16F_LINEAR)
		return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_set_image: unknown format");
	if (index >= ds->n_images) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_set_image: index past n_images");
	HIP_TRY(hipSetDevice(ds->ctx->device));
	hipStream_t s = (hipStream_t)stream;
	const size_t n_pixels = (size_t)ds->width * ds->height;
	uint64_t* dst = ds->d_images.get() + (size_t)index * n_pixels;
	const size_t bytes_per_pixel = format == NRS_IMAGE_RGBA8_SRGB ? 4 : (format == NRS_IMAGE_RGBA32F_LINEAR ? 16 : 8);
	if (format == NRS_IMAGE_RGBA16F_LINEAR) { // copied as it is
		HIP_TRY(hipMemcpyAsync(dst, pixels, n_pixels * 8, is_device_pointer ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
		if (!is_device_pointer) HIP_TRY(hipStreamSynchronize(s));
	} else {
		const void* src = pixels;
		if (!is_device_pointer) { // through the dataset's staging buffer: allocated once, for the widest format
			if (!ds->d_staging.get()) HIP_TRY(ds->d_staging.alloc(n_pixels * 16));
			HIP_TRY(hipMemcpyAsync(ds->d_staging.get(), pixels, n_pixels * bytes_per_pixel, hipMemcpyHostToDevice, s));
			HIP_TRY(hipStreamSynchronize(s)); // the caller's pixels have been read
			src = ds->d_staging.get();
		}
		NRS_LAUNCH(launch_dataset_convert(format, src, dst, n_pixels, flags, mask_color, stream));
	}
	if (!ds->image_set[index]) { ds->image_set[index] = 1; ds->n_images_set += 1; }
	return NRS_OK;
}

int nrs_dataset_get_image(nrs_dataset* ds, uint32_t index, void* h_out_fp16) {
	if (!ds || !h_out_fp16) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_get_image: NULL argument");
	if (index >= ds->n_images) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_get_image: index past n_images");
	if (!ds->image_set[index]) return fail(NRS_ERR_STATE, "nrs_dataset_get_image: the image has never been set (nrs_dataset_set_image)");
	HIP_TRY(hipSetDevice(ds->ctx->device));
	HIP_TRY(hipDeviceSynchronize());
	const size_t n_pixels = (size_t)ds->width * ds->height;
	HIP_TRY(hipMemcpy(h_out_fp16, ds->d_images.get() + (size_t)index * n_pixels, n_pixels * 8, hipMemcpyDeviceToHost));
	return NRS_OK;
}

int nrs_dataset_set_camera(nrs_dataset* ds, uint32_t index, const nrs_training_camera* cam) {
	if (!ds || !cam) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_set_camera: NULL argument");
	if (cam->struct_size != sizeof(nrs_training_camera)) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_set_camera: camera->struct_size is not sizeof(nrs_training_camera)");
	if (cam->distortion_mode > 2u) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_set_camera: unknown distortion_mode");
	float rec[kCameraWords];
	std::memcpy(rec, cam->xform_start, sizeof(rec)); // the record is the struct behind its struct_size (nrs_dataset.h)
	for (uint32_t k = 0; k < kCameraWords; ++k)
		if (k != 32 && !std::isfinite(rec[k])) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_set_camera: a camera entry is not finite");
	if (!(cam->focal_length[0] > 0.f) || !(cam->focal_length[1] > 0.f)) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_set_camera: focal_length is not positive");
	if (index >= ds->n_images) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_set_camera: index past n_images");
	std::memcpy(ds->cameras.data() + (size_t)index * kCameraWords, rec, sizeof(rec));
	ds->cameras_dirty = true;
	if (!ds->camera_set[index]) { ds->camera_set[index] = 1; ds->n_cameras_set += 1; }
	return NRS_OK;
}

int nrs_dataset_rays(nrs_dataset* ds, void* stream, const nrs_dataset_rays_params* p, uint32_t n_rays, float* d_rays, float* d_jitter, float* d_target_rgba,
                     float* d_background, uint32_t* d_pixels) {
	if (!ds || !p) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_rays: NULL argument");
	if (p->struct_size != sizeof(nrs_dataset_rays_params)) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_rays: params->struct_size is not sizeof(nrs_dataset_rays_params)");
	if (n_rays && (!d_rays || !d_jitter || !d_target_rgba || (p->random_bg_color && !d_background))) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_rays: NULL output");
	NRS_TRY(check_ray_count(n_rays, "nrs_dataset_rays", " (the generator's limit)"));
	NRS_TRY(check_complete(ds, "nrs_dataset_rays"));
	if (n_rays == 0) return NRS_OK;
	HIP_TRY(hipSetDevice(ds->ctx->device));
	NRS_TRY(send_cameras(ds, (hipStream_t)stream));
	DatasetRaysArgs a{};
	a.n_rays = n_rays; a.n_rays_total = p->n_rays_total; a.n_images = ds->n_images; a.width = ds->width; a.height = ds->height;
	a.rng_state = p->rng_state; a.rng_inc = p->rng_inc; a.snap = p->snap_to_pixel_centers ? 1u : 0u; a.random_bg = p->random_bg_color ? 1u : 0u;
	a.images = ds->d_images.get(); a.cameras = ds->d_cameras.get();
	a.rays = d_rays; a.jitter = d_jitter; a.target = d_target_rgba; a.background = d_background; a.pixels = d_pixels;
	NRS_LAUNCH(launch_dataset_rays(a, stream));
	return NRS_OK;
}

// ---- the training error map (include/nrs.h) ---------------------------------------------------------------------------------------------------------------
static int check_map_resolution(const nrs_dataset* ds, uint32_t res_x, uint32_t res_y, const char* who) {
	if (res_x < 2 || res_y < 2 || res_x > std::min(ds->width, NRS_ERROR_MAP_MAX_RESOLUTION) || res_y > std::min(ds->height, NRS_ERROR_MAP_MAX_RESOLUTION))
		return fail(NRS_ERR_INVALID_ARG, std::string(who) + ": the map's resolution must lie in [2, min(image resolution, 1024)] on each axis");
	if ((uint64_t)ds->n_images * res_y > 0x7fffffffull) return fail(NRS_ERR_INVALID_ARG, std::string(who) + ": n_images x res_y does not fit 31 bits");
	return NRS_OK;
}
// the cells for this resolution: the buffer is kept while its size stays (the caller fills it)
static int size_map(nrs_dataset* ds, uint32_t res_x, uint32_t res_y) {
	const size_t n = (size_t)ds->n_images * res_y * res_x;
	if (ds->d_error_map.get() && ds->d_error_map.count() == n) {
		ds->map_res_x = res_x; ds->map_res_y = res_y;
		return NRS_OK;
	}
	HIP_TRY(hipDeviceSynchronize()); // a launch may still read the buffer that goes
	ds->map_res_x = ds->map_res_y = 0;
	HIP_TRY(ds->d_error_map.alloc(n));
	ds->map_res_x = res_x; ds->map_res_y = res_y;
	return NRS_OK;
}

int nrs_dataset_error_map_reset(nrs_dataset* ds, uint32_t res_x, uint32_t res_y, void* stream) {
	if (!ds) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_error_map_reset: NULL argument");
	NRS_TRY(check_map_resolution(ds, res_x, res_y, "nrs_dataset_error_map_reset"));
	HIP_TRY(hipSetDevice(ds->ctx->device));
	NRS_TRY(size_map(ds, res_x, res_y));
	HIP_TRY(hipMemsetAsync(ds->d_error_map.get(), 0, ds->d_error_map.count() * sizeof(uint64_t), (hipStream_t)stream));
	return NRS_OK;
}

uint32_t nrs_error_map_resolution(uint32_t steps_between, uint32_t rays_per_batch, uint32_t n_images, uint32_t image_resolution) {
	if (n_images == 0 || image_resolution < 2) return 0;
	const uint32_t n_samples_per_image = (steps_between * rays_per_batch) / n_images; // 32-bit, as the reference's
	const int res = (int)(sqrtf(sqrtf((float)n_samples_per_image)) * 3.5f);
	return (uint32_t)std::min(std::max(res, 2), (int)std::min(image_resolution, NRS_ERROR_MAP_MAX_RESOLUTION));
}

int nrs_dataset_error_map_set(nrs_dataset* ds, uint32_t res_x, uint32_t res_y, const float* h_data_f32) {
	if (!ds || !h_data_f32) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_error_map_set: NULL argument");
	NRS_TRY(check_map_resolution(ds, res_x, res_y, "nrs_dataset_error_map_set"));
	const size_t n = (size_t)ds->n_images * res_y * res_x;
	std::vector<uint64_t> cells(n);
	for (size_t k = 0; k < n; ++k) cells[k] = error_cell_quantise(h_data_f32[k]);
	HIP_TRY(hipSetDevice(ds->ctx->device));
	HIP_TRY(hipDeviceSynchronize());
	NRS_TRY(size_map(ds, res_x, res_y));
	HIP_TRY(hipMemcpy(ds->d_error_map.get(), cells.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice));
	return NRS_OK;
}

int nrs_dataset_error_map_get(nrs_dataset* ds, int what, void* h_out, size_t* count) {
	if (!ds) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_error_map_get: NULL argument");
	if (what < NRS_ERROR_MAP_FLOAT || what > NRS_ERROR_MAP_CELLS) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_error_map_get: unknown `what`");
	const bool map = what == NRS_ERROR_MAP_FLOAT || what == NRS_ERROR_MAP_CELLS;
	if (map && !ds->map_res_x) return fail(NRS_ERR_STATE, "nrs_dataset_error_map_get: there is no map (nrs_dataset_error_map_reset)");
	if (!map && !ds->cdf_valid) return fail(NRS_ERR_STATE, "nrs_dataset_error_map_get: there are no valid CDFs (nrs_dataset_error_map_build_cdfs)");
	const void* src = nullptr;
	size_t n = 0;
	switch (what) {
	case NRS_ERROR_MAP_FLOAT: case NRS_ERROR_MAP_CELLS: src = ds->d_error_map.get(); n = (size_t)ds->n_images * ds->map_res_y * ds->map_res_x; break;
	case NRS_ERROR_MAP_CDF_X_COND_Y: src = ds->d_cdf_x_cond_y.get(); n = (size_t)ds->n_images * ds->cdf_res_y * ds->cdf_res_x; break;
	case NRS_ERROR_MAP_CDF_Y: src = ds->d_cdf_y.get(); n = (size_t)ds->n_images * ds->cdf_res_y; break;
	case NRS_ERROR_MAP_CDF_IMG: src = ds->d_cdf_img.get(); n = ds->n_images; break;
	default: src = ds->d_pmf_img.get(); n = ds->n_images; break;
	}
	if (count) *count = n;
	if (!h_out) return NRS_OK;
	HIP_TRY(hipSetDevice(ds->ctx->device));
	HIP_TRY(hipDeviceSynchronize());
	if (what == NRS_ERROR_MAP_FLOAT) { // the reference's float map, formed where it is read
		std::vector<uint64_t> cells(n);
		HIP_TRY(hipMemcpy(cells.data(), src, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
		for (size_t k = 0; k < n; ++k) ((float*)h_out)[k] = error_cell_to_float(cells[k]);
		return NRS_OK;
	}
	HIP_TRY(hipMemcpy(h_out, src, n * (what == NRS_ERROR_MAP_CELLS ? sizeof(uint64_t) : sizeof(float)), hipMemcpyDeviceToHost));
	return NRS_OK;
}

int nrs_dataset_error_map_accumulate(nrs_dataset* ds, void* stream, uint32_t n_rays, const uint32_t* d_ray_counter, const uint32_t* d_ray_indices, const float* d_loss,
                                     const float* d_xy, const uint32_t* d_pixels, const float* d_pdf, float* d_loss_weighted) {
	if (!ds) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_error_map_accumulate: NULL argument");
	if (n_rays && (!d_ray_counter || !d_ray_indices || !d_loss || !d_xy || !d_pixels)) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_error_map_accumulate: NULL input");
	NRS_TRY(check_ray_count(n_rays, "nrs_dataset_error_map_accumulate", " (what the cells hold without a wrap)"));
	if (!ds->map_res_x) return fail(NRS_ERR_STATE, "nrs_dataset_error_map_accumulate: there is no map (nrs_dataset_error_map_reset)");
	if (n_rays == 0) return NRS_OK;
	HIP_TRY(hipSetDevice(ds->ctx->device));
	ErrorMapAccumulateArgs a{};
	a.n_rays = n_rays; a.n_images = ds->n_images; a.res_x = ds->map_res_x; a.res_y = ds->map_res_y;
	a.ray_counter = d_ray_counter; a.ray_indices = d_ray_indices; a.loss = d_loss; a.xy = d_xy; a.pixels = d_pixels; a.pdf = d_pdf; a.loss_weighted = d_loss_weighted;
	a.cells = ds->d_error_map.get();
	NRS_LAUNCH(launch_error_map_accumulate(a, stream));
	return NRS_OK;
}

int nrs_dataset_error_map_build_cdfs(nrs_dataset* ds, void* stream) {
	if (!ds) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_error_map_build_cdfs: NULL argument");
	if (!ds->map_res_x) return fail(NRS_ERR_STATE, "nrs_dataset_error_map_build_cdfs: there is no map (nrs_dataset_error_map_reset)");
	HIP_TRY(hipSetDevice(ds->ctx->device));
	const size_t n_rows = (size_t)ds->n_images * ds->map_res_y, n_cells = n_rows * ds->map_res_x;
	if (ds->d_cdf_x_cond_y.count() != n_cells || ds->d_cdf_y.count() != n_rows || !ds->d_cdf_img.get()) {
		ds->cdf_valid = false;
		HIP_TRY(hipDeviceSynchronize()); // a launch may still read the CDFs that go
		HIP_TRY(ds->d_cdf_x_cond_y.alloc(n_cells));
		HIP_TRY(ds->d_cdf_y.alloc(n_rows));
		if (!ds->d_cdf_img.get()) {
			HIP_TRY(ds->d_cdf_img.alloc(ds->n_images));
			HIP_TRY(ds->d_pmf_img.alloc(ds->n_images));
			HIP_TRY(ds->d_img_total.alloc(ds->n_images));
		}
	}
	ds->cdf_valid = false;
	NRS_LAUNCH(launch_error_map_cdfs(ds->n_images, ds->map_res_y, ds->map_res_x, ds->d_error_map.get(), ds->d_cdf_x_cond_y.get(), ds->d_cdf_y.get(), ds->d_img_total.get(),
	                                 ds->d_cdf_img.get(), ds->d_pmf_img.get(), stream));
	ds->cdf_res_x = ds->map_res_x; ds->cdf_res_y = ds->map_res_y;
	ds->cdf_valid = true;
	return NRS_OK;
}

int nrs_error_map_cdfs_host(uint32_t n_images, uint32_t res_y, uint32_t res_x, const float* data, float* cdf_x_cond_y, float* cdf_y, float* cdf_img, float* pmf_img) {
	if (!data || !cdf_x_cond_y || !cdf_y || !cdf_img || !pmf_img) return fail(NRS_ERR_INVALID_ARG, "nrs_error_map_cdfs_host: NULL argument");
	if (n_images == 0 || res_x == 0 || res_y == 0) return fail(NRS_ERR_INVALID_ARG, "nrs_error_map_cdfs_host: n_images or a resolution is 0");
	constexpr float MIN_PDF = 0.01f, MIN_PMF = 0.1f;
	for (uint32_t img = 0; img < n_images; ++img) {
		float* cy = cdf_y + (size_t)img * res_y;
		for (uint32_t y = 0; y < res_y; ++y) { // construct_cdf_2d
			const float* d = data + ((size_t)img * res_y + y) * res_x;
			float* c = cdf_x_cond_y + ((size_t)img * res_y + y) * res_x;
			float cum = 0;
			for (uint32_t x = 0; x < res_x; ++x) {
				cum += d[x] + 1e-10f;
				c[x] = cum;
			}
			cy[y] = cum;
			const float norm = 1.0f / cum;
			for (uint32_t x = 0; x < res_x; ++x) c[x] = (1.0f - MIN_PDF) * c[x] * norm + MIN_PDF * (float)(x + 1) / (float)res_x;
		}
		float cum = 0; // construct_cdf_1d
		for (uint32_t y = 0; y < res_y; ++y) {
			cum += cy[y];
			cy[y] = cum;
		}
		pmf_img[img] = cum;
		const float norm = 1.0f / cum;
		for (uint32_t y = 0; y < res_y; ++y) cy[y] = (1.0f - MIN_PDF) * cy[y] * norm + MIN_PDF * (float)(y + 1) / (float)res_y;
	}
	float cum = 0; // the host loop of train_nerf
	for (uint32_t i = 0; i < n_images; ++i) {
		cum += pmf_img[i];
		cdf_img[i] = cum;
	}
	const float norm = 1.0f / cum;
	for (uint32_t i = 0; i < n_images; ++i) {
		pmf_img[i] = (1.0f - MIN_PMF) * pmf_img[i] * norm + MIN_PMF / (float)n_images;
		cdf_img[i] = (1.0f - MIN_PMF) * cdf_img[i] * norm + MIN_PMF * (float)(i + 1) / (float)n_images;
	}
	return NRS_OK;
}

int nrs_dataset_rays_ex(nrs_dataset* ds, void* stream, const nrs_dataset_rays_ex_params* p, uint32_t n_rays, float* d_rays, float* d_jitter, float* d_target_rgba,
                        float* d_background, uint32_t* d_pixels, float* d_xy, float* d_pdf) {
	if (!ds || !p) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_rays_ex: NULL argument");
	if (p->struct_size != sizeof(nrs_dataset_rays_ex_params)) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_rays_ex: params->struct_size is not sizeof(nrs_dataset_rays_ex_params)");
	if (n_rays && (!d_rays || !d_jitter || !d_target_rgba || (p->random_bg_color && !d_background))) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_rays_ex: NULL output");
	NRS_TRY(check_ray_count(n_rays, "nrs_dataset_rays_ex", " (the generator's limit)"));
	NRS_TRY(check_complete(ds, "nrs_dataset_rays_ex"));
	if ((p->sample_images_by_error || p->sample_pixels_by_error) && !ds->cdf_valid)
		return fail(NRS_ERR_STATE, "nrs_dataset_rays_ex: sampling by error without valid CDFs (nrs_dataset_error_map_build_cdfs)");
	if (n_rays == 0) return NRS_OK;
	HIP_TRY(hipSetDevice(ds->ctx->device));
	NRS_TRY(send_cameras(ds, (hipStream_t)stream));
	DatasetRaysArgs a{};
	a.n_rays = n_rays; a.n_rays_total = p->n_rays_total; a.n_images = ds->n_images; a.width = ds->width; a.height = ds->height;
	a.rng_state = p->rng_state; a.rng_inc = p->rng_inc; a.snap = p->snap_to_pixel_centers ? 1u : 0u; a.random_bg = p->random_bg_color ? 1u : 0u;
	a.images = ds->d_images.get(); a.cameras = ds->d_cameras.get();
	a.rays = d_rays; a.jitter = d_jitter; a.target = d_target_rgba; a.background = d_background; a.pixels = d_pixels;
	a.by_images = p->sample_images_by_error ? 1u : 0u; a.by_pixels = p->sample_pixels_by_error ? 1u : 0u;
	a.cdf_res_x = ds->cdf_res_x; a.cdf_res_y = ds->cdf_res_y;
	a.cdf_x_cond_y = ds->d_cdf_x_cond_y.get(); a.cdf_y = ds->d_cdf_y.get(); a.cdf_img = ds->d_cdf_img.get();
	a.xy = d_xy; a.pdf = d_pdf;
	NRS_LAUNCH(launch_dataset_rays_ex(a, stream));
	return NRS_OK;
}

int nrs_dataset_mark_untrained(nrs_model* m, nrs_dataset* ds, int clear_visible_voxels, void* stream) {
	if (!m || !ds) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_mark_untrained: NULL argument");
	if (m->ctx != ds->ctx) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_mark_untrained: the model and the dataset belong to different contexts");
	NRS_TRY(check_complete(ds, "nrs_dataset_mark_untrained"));
	HIP_TRY(hipSetDevice(ds->ctx->device));
	NRS_TRY(send_cameras(ds, (hipStream_t)stream));
	NRS_LAUNCH(launch_mark_untrained(m->d_density_grid.get(), ds->n_images, ds->d_cameras.get(), ds->width, ds->height, clear_visible_voxels, stream));
	return model_refresh_bitfield(m, stream);
}

} // extern "C"
