// nrs_dataset.hip -- the dataset on the device (gfx950, wave64).
//
//   dataset_convert_*       the loader's image conversion: from_rgba32<__half> (common_device.cuh:513-540), from_fullp (src/nerf_loader.cu:62).
//   dataset_rays_kernel     generate_training_samples_nerf up to the ray (tn:1087-1186) and the target / background look-ups of the loss kernel (tn:1777-1806).
//   mark_untrained_kernel   mark_untrained_density_grid (tn:353-400).
#include <hip/hip_runtime.h>
#include "nrs_dataset.h"
#include "nrs_launch.h"
#include "nrs_device.cuh"

namespace nrs {

// ---- image conversion ------------------------------------------------------------------------------------------------------------------------------
// srgb_to_linear as the LOADER evaluates it (common_device.cuh:31-37): a division and powf, not the render path's exp2 / log2 form -- an image is converted once, and
// its fp16 pixels are compared with the reference arithmetic to the rounding step.
__device__ __forceinline__ float loader_srgb_to_linear(float s) {
	if (s <= 0.04045f) return s / 12.92f;
	return powf((s + 0.055f) / 1.055f, 2.4f);
}
__device__ __forceinline__ uint64_t pack_half4(float r, float g, float b, float a) {
	union { _Float16 h[4]; uint64_t u; } p;
	p.h[0] = (_Float16)r; p.h[1] = (_Float16)g; p.h[2] = (_Float16)b; p.h[3] = (_Float16)a;
	return p.u;
}
__global__ __launch_bounds__(256) void dataset_convert_rgba8_kernel(uint64_t n_pixels, const uint32_t* __restrict__ pixels, uint64_t* __restrict__ out, uint32_t white_2_transparent,
                                                                    uint32_t black_2_transparent, uint32_t mask_color) {
	const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n_pixels) return;
	const uint32_t w = pixels[i];
	const uint32_t r = w & 0xffu, g = (w >> 8) & 0xffu, b = (w >> 16) & 0xffu, a = w >> 24;
	float alpha = (float)a * (1.0f / 255.0f);
	if (white_2_transparent && r == 255u && g == 255u && b == 255u) alpha = 0.f;
	if (black_2_transparent && r == 0u && g == 0u && b == 0u) alpha = 0.f;
	uint64_t o = pack_half4(loader_srgb_to_linear((float)r * (1.0f / 255.0f)) * alpha, loader_srgb_to_linear((float)g * (1.0f / 255.0f)) * alpha,
	                        loader_srgb_to_linear((float)b * (1.0f / 255.0f)) * alpha, alpha);
	if (mask_color != 0u && mask_color == w) o = pack_half4(-1.0f, -1.0f, -1.0f, -1.0f);
	out[i] = o;
}
__global__ __launch_bounds__(256) void dataset_convert_f32_kernel(uint64_t n_pixels, const float4* __restrict__ pixels, uint64_t* __restrict__ out) {
	const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n_pixels) return;
	const float4 p = pixels[i];
	out[i] = pack_half4(p.x, p.y, p.z, p.w);
}
int launch_dataset_convert(int format, const void* src, uint64_t* dst, uint64_t n_pixels, uint32_t flags, uint32_t mask_color, void* stream) {
	hipStream_t s = (hipStream_t)stream;
	const dim3 grid((uint32_t)((n_pixels + 255) / 256));
	if (format == NRS_IMAGE_RGBA8_SRGB)
		hipLaunchKernelGGL(dataset_convert_rgba8_kernel, grid, dim3(256), 0, s, n_pixels, (const uint32_t*)src, dst, flags & NRS_IMAGE_WHITE_TRANSPARENT,
		                   flags & NRS_IMAGE_BLACK_TRANSPARENT, mask_color);
	else
		hipLaunchKernelGGL(dataset_convert_f32_kernel, grid, dim3(256), 0, s, n_pixels, (const float4*)src, dst);
	NRS_LAUNCH_CHECK("dataset_convert launch");
	return NRS_OK;
}

// ---- pixel rays and their targets --------------------------------------------------------------------------------------------------------------------
// The ray through (u, v) of the camera record `c` at motion-blur time mb (tn:1135-1185).  C is a pointer to the record's 40 words in the constant address space (the
// record is the same in every lane: scalar loads) or in the global one (per lane); the arithmetic on the loaded words is the same text, so the bits are too.
template <typename C>
__device__ __forceinline__ void dataset_ray(C c, uint32_t W, uint32_t H, float u, float v, float mb, f3& o, f3& d) {
	const float pixel_t = c[28] + c[29] * u + c[30] * v + c[31] * mb; // get_xform_given_rolling_shutter, common_device.cuh:226-229
	float cam[12];
	#pragma unroll
	for (int i = 0; i < 12; ++i) {
		const float start = c[i];
		cam[i] = start + (c[12 + i] - start) * pixel_t;
	}
	o = {cam[9], cam[10], cam[11]};
	const uint32_t mode = __float_as_uint(c[32]);
	float prm[7];
	#pragma unroll
	for (int k = 0; k < 7; ++k) prm[k] = c[33 + k];
	f3 dir = mk3(0.f, 0.f, 1.f); // f_theta_undistortion's error direction here (tn:1170)
	if (mode == 2u) {
		(void)f_theta_undistortion(prm, u, v, c[26], c[27], dir);
	} else {
		dir = {(u - c[26]) * (float)W / c[24], (v - c[27]) * (float)H / c[25], 1.0f};
		if (mode == 1u) iterative_camera_undistortion(prm, dir.x, dir.y);
	}
	d = mat3_mul(cam, dir);
	const float n = sqrtf(dot3(d, d));
	d = {d.x / n, d.y / n, d.z / n};
}

__global__ __launch_bounds__(256) void dataset_rays_kernel(const DatasetRaysArgs a) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= a.n_rays) return;
	const uint32_t img = (((i + a.n_rays_total) * a.n_images) / a.n_rays) % a.n_images; // image_idx, tn:1072: 32-bit, the product wraps
	Pcg32 rng{a.rng_state, a.rng_inc};
	// N_MAX_RANDOM_SAMPLES_PER_RAY.  The plain per-lane skip loop: composing it from a wave-uniform skip and a per-lane step out of a table built once per workgroup,
	// as grid_refresh_kernel does, was measured and lost (profiles/dataset_rays.md): a thread lives for one ray here, so the table and its barrier are never paid back.
	rng.advance((uint64_t)(i * 8u));
	const float W = (float)a.width, H = (float)a.height;
	float u = rng.next_float(), v = rng.next_float(); // draws 0, 1
	if (a.snap) { // tn:1047
		u = ((float)max(min((int)(u * W), (int)a.width - 1), 0) + 0.5f) / W;
		v = ((float)max(min((int)(v * H), (int)a.height - 1), 0) + 0.5f) / H;
	}
	const uint32_t px = (uint32_t)max(min((int)(u * W), (int)a.width - 1), 0), py = (uint32_t)max(min((int)(v * H), (int)a.height - 1), 0); // image_pos, tn:1075
	const uint32_t pixel = px + py * a.width;
	union { uint64_t u; _Float16 h[4]; } texel;
	texel.u = a.images[(uint64_t)pixel + (uint64_t)img * ((uint64_t)a.width * a.height)]; // pixel_idx, tn:1079
	const bool masked = (float)texel.h[0] < 0.0f; // tn:1127
	const float mb = rng.next_float();     // draw 2: motionblur_time
	const float jitter = rng.next_float(); // draw 3
	const float bg2 = rng.next_float();    // draw 4

	f3 o, d;
	// consecutive rays share an image (n_rays / n_images in a row): where the whole wave does, its record comes in through scalar loads (measured: profiles/dataset_rays.md)
	const uint32_t img0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)img);
	if (__all(img == img0)) dataset_ray((const NRS_CONSTANT float*)a.cameras + (size_t)img0 * kCameraWords, a.width, a.height, u, v, mb, o, d);
	else dataset_ray((const NRS_GLOBAL float*)a.cameras + (size_t)img * kCameraWords, a.width, a.height, u, v, mb, o, d);
	if (masked) d = mk3(0.f, 0.f, 0.f); // a dead ray: nrs_training_samples gives it no samples

	float2* r = reinterpret_cast<float2*>(a.rays + (size_t)i * 6);
	r[0] = make_float2(o.x, o.y); r[1] = make_float2(o.z, d.x); r[2] = make_float2(d.y, d.z);
	a.jitter[i] = jitter;
	reinterpret_cast<float4*>(a.target)[i] = masked ? make_float4(0.f, 0.f, 0.f, 0.f) : make_float4((float)texel.h[0], (float)texel.h[1], (float)texel.h[2], (float)texel.h[3]);
	if (a.random_bg) { // random_val_3d behind xy of the re-seeded generator (tn:1780-1791): draws 2, 3, 4
		float* b = a.background + (size_t)i * 3;
		b[0] = mb; b[1] = jitter; b[2] = bg2;
	}
	if (a.pixels) reinterpret_cast<uint2*>(a.pixels)[i] = make_uint2(img, pixel);
}
int launch_dataset_rays(const DatasetRaysArgs& a, void* stream) {
	if (a.n_rays == 0) return NRS_OK;
	hipLaunchKernelGGL(dataset_rays_kernel, dim3((a.n_rays + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
	NRS_LAUNCH_CHECK("dataset_rays_kernel launch");
	return NRS_OK;
}

// ---- mark_untrained_density_grid (tn:353-400) --------------------------------------------------------------------------------------------------------
// One thread per cell; the camera loop is the same in every lane, so the records come in through scalar loads.
__global__ __launch_bounds__(256) void mark_untrained_kernel(uint32_t n_elements, float* __restrict__ grid_out, uint32_t n_images, const float* __restrict__ cameras,
                                                             uint32_t width, uint32_t height, uint32_t clear_visible_voxels) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n_elements) return;
	const uint32_t level = i / kGridVol, pos_idx = i % kGridVol;
	const float x = (float)morton3D_invert(pos_idx >> 0), y = (float)morton3D_invert(pos_idx >> 1), z = (float)morton3D_invert(pos_idx >> 2);
	const float half_resx = (float)width * 0.5f, half_resy = (float)height * 0.5f;
	const float s = __uint_as_float((127u + level) << 23); // scalbnf(1, level)
	const f3 pos = {((x + 0.5f) / (float)kGrid - 0.5f) * s + 0.5f, ((y + 0.5f) / (float)kGrid - 0.5f) * s + 0.5f, ((z + 0.5f) / (float)kGrid - 0.5f) * s + 0.5f};
	const float voxel_radius = 0.5f * NRS_SQRT3 * s / (float)kGrid;
	bool seen = false;
	for (uint32_t j = 0; j < n_images && !seen; ++j) {
		const NRS_CONSTANT float* c = (const NRS_CONSTANT float*)cameras + (size_t)j * kCameraWords;
		if (__float_as_uint(c[32]) == 2u) { seen = true; break; } // f-theta: "not supported for now" -- counts as seeing everything
		const f3 ploc = {pos.x - c[9], pos.y - c[10], pos.z - c[11]};
		const float cx = dot3(ploc, mk3(c[0], c[1], c[2])), cy = dot3(ploc, mk3(c[3], c[4], c[5])), cz = dot3(ploc, mk3(c[6], c[7], c[8]));
		if (cz > 0.f && fabsf(cx) - voxel_radius < cz / c[24] * half_resx && fabsf(cy) - voxel_radius < cz / c[25] * half_resy) seen = true;
	}
	if (clear_visible_voxels || (grid_out[i] < 0) != !seen) grid_out[i] = seen ? 0.f : -1.f;
}
int launch_mark_untrained(float* d_grid, uint32_t n_images, const float* d_cameras, uint32_t width, uint32_t height, int clear_visible, void* stream) {
	const uint32_t n = kGridVol * kCascades;
	hipLaunchKernelGGL(mark_untrained_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, d_grid, n_images, d_cameras, width, height,
	                   clear_visible ? 1u : 0u);
	NRS_LAUNCH_CHECK("mark_untrained_kernel launch");
	return NRS_OK;
}

} // namespace nrs
