// nrs_api_dataset.cpp -- the dataset behind the C-ABI: create / destroy, images (converted on the device), cameras (kept on the host, sent in one block), the pixel
// rays of a training step and mark_untrained.  Everything that can be refused is refused before the first HIP call.
#include "nrs_handles.h"
#include "nrs_dataset.h"
#include "nrs_train.h"

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
	if (n_rays > kTrainMaxRays) return fail(NRS_ERR_INVALID_ARG, "nrs_dataset_rays: more than 2^21 rays (the generator's limit)");
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
