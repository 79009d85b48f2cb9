// nrs_dataset.hip -- the dataset on the device (gfx950, wave64).
//
//   dataset_convert_*       the loader's image conversion: from_rgba32<__half> (common_device.cuh:513-540), from_fullp (src/nerf_loader.cu:62).
//   dataset_rays_kernel     generate_training_samples_nerf up to the ray (tn:1087-1186) and the target / background look-ups of the loss kernel (tn:1777-1806).
//   dataset_rays_kernel<true>    the same with the image drawn from cdf_img (tn:1052-1064) and the pixel from cdf_y / cdf_x_cond_y (tn:983-1012): nrs_dataset_rays_ex.
//   error_map_accumulate_kernel  the loss kernel's deposits into the error map (tn:1861-1886), in 64-bit fixed point.
//   error_map_cdf_kernel         construct_cdf_2d (tn:2620), construct_cdf_1d (tn:2650) and train_nerf's host loop over the images (tn:3811-3822).
//   mark_untrained_kernel   mark_untrained_density_grid (tn:353-400).
#include <hip/hip_runtime.h>
#include "../../include/nrs.h"
#include "nrs_internal.h"
#include "nrs_launch.h"
#include "nrs_dataset.h"
#include "nrs_train.h"
#include "nrs_cells.h"
#include "nrs_vec.cuh"
#include "nrs_grid_math.cuh"
#include "nrs_random.cuh"
#include "nrs_camera.cuh"

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

// binary_search (common.h:187-210): the first index whose entry is not < val, capped at length - 1 (length >= 1)
__device__ __forceinline__ uint32_t cdf_search(float val, const float* __restrict__ data, uint32_t length) {
	uint32_t first = 0, count = length;
	while (count > 0) {
		const uint32_t step = count / 2, it = first + step;
		if (data[it] < val) { first = it + 1; count -= step + 1; }
		else count = step;
	}
	return min(first, length - 1);
}

// EX = false is nrs_dataset_rays: the `cdf == nullptr` branches of the reference and nothing else.  EX = true is its twin for nrs_dataset_rays_ex: the image from
// cdf_img (image_idx, tn:1052-1064), the pixel from cdf_y and cdf_x_cond_y (sample_cdf_2d, tn:983-1012), each behind its switch, and the two outputs xy and pdf.  The
// generator's draws are the same five in the same order in both.
template <bool EX>
__global__ __launch_bounds__(256) void dataset_rays_kernel(const DatasetRaysArgs a) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= a.n_rays) return;
	uint32_t img = (((i + a.n_rays_total) * a.n_images) / a.n_rays) % a.n_images; // image_idx, tn:1072: 32-bit, the product wraps
	float img_pdf = 1.0f, xy_pdf = 1.0f;
	if (EX && a.by_images) {
		img = cdf_search(ld_random_val(i + a.n_rays_total, 0xdeadbeefu), a.cdf_img, a.n_images);
		const float prev = img > 0 ? a.cdf_img[img - 1] : 0.0f;
		img_pdf = (a.cdf_img[img] - prev) * (float)a.n_images;
	}
	Pcg32 rng{a.rng_state, a.rng_inc};
	// N_MAX_RANDOM_SAMPLES_PER_RAY.  The plain per-lane skip loop: composing it from a wave-uniform skip and a per-lane step out of a table built once per workgroup,
	// as grid_refresh_kernel does, was measured and lost (profiles/dataset_rays.md): a thread lives for one ray here, so the table and its barrier are never paid back.
	rng.advance((uint64_t)(i * 8u));
	const float W = (float)a.width, H = (float)a.height;
	float u = rng.next_float(), v = rng.next_float(); // draws 0, 1
	if (EX && a.by_pixels) { // sample_cdf_2d: UNIFORM_SAMPLING_FRACTION = 0.5 of the rays stay uniform, and xy_pdf is the density of the OTHER half alone (as in the reference)
		if (u < 0.5f) {
			u /= 0.5f;
		} else {
			u = (u - 0.5f) / (1.0f - 0.5f);
			const float* cy = a.cdf_y + (size_t)img * a.cdf_res_y;
			const uint32_t row = cdf_search(v, cy, a.cdf_res_y);
			float prev = row > 0 ? cy[row - 1] : 0.0f;
			const float pmf_y = cy[row] - prev;
			v = (v - prev) / pmf_y;
			const float* cx = a.cdf_x_cond_y + ((size_t)img * a.cdf_res_y + row) * a.cdf_res_x;
			const uint32_t col = cdf_search(u, cx, a.cdf_res_x);
			prev = col > 0 ? cx[col - 1] : 0.0f;
			const float pmf_x = cx[col] - prev;
			u = (u - prev) / pmf_x;
			xy_pdf = pmf_x * pmf_y * (float)(int)(a.cdf_res_x * a.cdf_res_y);
			u = ((float)col + u) / (float)(int)a.cdf_res_x;
			v = ((float)row + v) / (float)(int)a.cdf_res_y;
		}
	}
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
	if (EX) {
		if (a.xy) reinterpret_cast<float2*>(a.xy)[i] = make_float2(u, v);
		if (a.pdf) a.pdf[i] = img_pdf * xy_pdf;
	}
}
int launch_dataset_rays(const DatasetRaysArgs& a, void* stream) {
	if (a.n_rays == 0) return NRS_OK;
	hipLaunchKernelGGL(dataset_rays_kernel<false>, dim3((a.n_rays + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
	NRS_LAUNCH_CHECK("dataset_rays_kernel launch");
	return NRS_OK;
}
int launch_dataset_rays_ex(const DatasetRaysArgs& a, void* stream) {
	if (a.n_rays == 0) return NRS_OK;
	hipLaunchKernelGGL(dataset_rays_kernel<true>, dim3((a.n_rays + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
	NRS_LAUNCH_CHECK("dataset_rays_kernel<ex> launch");
	return NRS_OK;
}

// ---- the error map: deposits (tn:1861-1886) -----------------------------------------------------------------------------------------------------------
// One deposit (include/nrs.h, deviation 1): error_cell_deposit (nrs_cells.h).
__global__ __launch_bounds__(256) void error_map_accumulate_kernel(const ErrorMapAccumulateArgs a) {
	const uint32_t s = blockIdx.x * 256 + threadIdx.x;
	if (s >= live_slots(a.ray_counter, a.n_rays)) return;
	const uint32_t i = a.ray_indices[s];
	if (i >= a.n_rays) return;
	const float loss = a.loss[s];
	const float p = a.pdf ? a.pdf[i] : 1.0f;
	if (a.loss_weighted) a.loss_weighted[s] = loss / p; // tn:1848 (may be a.loss itself: this thread's own slot, read above)
	const uint32_t img = a.pixels[2 * (size_t)i];
	if (img >= a.n_images) return;
	const float e = (loss * (float)a.n_rays) / p; // loss_output is mean_loss / n_rays, tn:1858
	const float2 xy = reinterpret_cast<const float2*>(a.xy)[i];
	const float rx = (float)(int)a.res_x, ry = (float)(int)a.res_y;
	const float px = fminf(fmaxf(xy.x * rx - 0.5f, 0.0f), rx - (1.0f + 1e-4f)), py = fminf(fmaxf(xy.y * ry - 0.5f, 0.0f), ry - (1.0f + 1e-4f));
	const int ix = (int)px, iy = (int)py;
	const float wx = px - (float)ix, wy = py - (float)iy;
	// res >= 2 and the clamp of pos put the cell into [0, res - 2] already; the clamp below acts for a NaN in xy alone (include/nrs.h, deviation 3)
	const uint32_t cx = (uint32_t)max(min(ix, (int)a.res_x - 2), 0), cy = (uint32_t)max(min(iy, (int)a.res_y - 2), 0);
	uint64_t* c = a.cells + ((size_t)img * a.res_y + cy) * a.res_x + cx;
	error_cell_deposit(c, (1 - wx) * (1 - wy) * e);
	error_cell_deposit(c + 1, wx * (1 - wy) * e);
	error_cell_deposit(c + a.res_x, (1 - wx) * wy * e);
	error_cell_deposit(c + a.res_x + 1, wx * wy * e);
}
int launch_error_map_accumulate(const ErrorMapAccumulateArgs& a, void* stream) {
	if (a.n_rays == 0) return NRS_OK;
	hipLaunchKernelGGL(error_map_accumulate_kernel, dim3((a.n_rays + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
	NRS_LAUNCH_CHECK("error_map_accumulate_kernel launch");
	return NRS_OK;
}

// ---- the error map: CDFs (construct_cdf_2d tn:2620, construct_cdf_1d tn:2650, the host loop of train_nerf tn:3811-3822) ------------------------------------
// One running sum per row, and the serial association of that sum is the definition -- so the chain is one lane's; what is parallel is everything around it.  The rows
// of all three stages are contiguous (row r starts at r * width), so a wave takes 64 consecutive rows, one per lane, and walks them in tiles of 16 columns: the 64
// lanes load the tile with 16 lanes to a row's segment (64 or 128 contiguous bytes each), every lane then walks ITS row's 16 entries out of LDS (17 words to a row:
// no bank is hit twice) and leaves the running sums there, and the 64 lanes store the tile as they loaded it.  The chain never waits for global memory.  With the
// totals known the block normalises its rows in one coalesced pass.
//   MODE 0: src = the cells [n_images * res_y rows][res_x]; the entry is (float)cell * 2^-32 + 1e-10f; total_out = cdf_y (unnormalised)
//   MODE 1: src = cdf = cdf_y [n_images rows][res_y], in place; total_out = the pictures' totals
//   MODE 2: src = the pictures' totals [1 row][n_images]; MIN_PMF = 0.1 in place of MIN_PDF = 0.01, and pmf_out
constexpr uint32_t kCdfTile = 16;
template <int MODE>
__global__ __launch_bounds__(64) void error_map_cdf_kernel(uint32_t n_rows, uint32_t width, const void* src, float* cdf, float* total_out, float* pmf_out) {
	__shared__ float tile[64][kCdfTile + 1];
	__shared__ float norm[64];
	const uint32_t lane = threadIdx.x, row0 = blockIdx.x * 64u, rows = min(64u, n_rows - row0);
	float cum = 0.0f;
	for (uint32_t c0 = 0; c0 < width; c0 += kCdfTile) {
		const uint32_t cw = min(kCdfTile, width - c0);
		#pragma unroll
		for (uint32_t k = 0; k < kCdfTile; ++k) {
			const uint32_t e = k * 64u + lane, r = e / kCdfTile, x = e % kCdfTile;
			if (r < rows && x < cw) {
				const size_t at = (size_t)(row0 + r) * width + c0 + x;
				tile[r][x] = MODE == 0 ? error_cell_to_float(((const uint64_t*)src)[at]) + 1e-10f : ((const float*)src)[at];
			}
		}
		__syncthreads();
		if (lane < rows)
			for (uint32_t x = 0; x < cw; ++x) {
				cum += tile[lane][x];
				tile[lane][x] = cum;
			}
		__syncthreads();
		#pragma unroll
		for (uint32_t k = 0; k < kCdfTile; ++k) {
			const uint32_t e = k * 64u + lane, r = e / kCdfTile, x = e % kCdfTile;
			if (r < rows && x < cw) cdf[(size_t)(row0 + r) * width + c0 + x] = tile[r][x];
		}
		__syncthreads();
	}
	if (lane < rows) {
		if (MODE != 2) total_out[row0 + lane] = cum;
		norm[lane] = 1.0f / cum; // __frcp_rn
	}
	__syncthreads();
	constexpr float kMin = MODE == 2 ? 0.1f : 0.01f; // MIN_PMF : MIN_PDF
	for (uint32_t e = lane; e < rows * width; e += 64u) { // (rows * width <= 64 * 1024, or one row of n_images)
		const uint32_t r = e / width, x = e % width;
		const size_t at = (size_t)row0 * width + e;
		cdf[at] = (1.0f - kMin) * cdf[at] * norm[r] + kMin * (float)(x + 1) / (float)width;
		if (MODE == 2) pmf_out[at] = (1.0f - kMin) * ((const float*)src)[at] * norm[r] + kMin / (float)width;
	}
}
int launch_error_map_cdfs(uint32_t n_images, uint32_t res_y, uint32_t res_x, const uint64_t* d_cells, float* d_cdf_x_cond_y, float* d_cdf_y, float* d_img_total,
                          float* d_cdf_img, float* d_pmf_img, void* stream) {
	hipStream_t s = (hipStream_t)stream;
	const uint32_t n_rows = n_images * res_y;
	hipLaunchKernelGGL(error_map_cdf_kernel<0>, dim3((n_rows + 63) / 64), dim3(64), 0, s, n_rows, res_x, (const void*)d_cells, d_cdf_x_cond_y, d_cdf_y, (float*)nullptr);
	NRS_LAUNCH_CHECK("error_map_cdf_kernel<0> launch");
	hipLaunchKernelGGL(error_map_cdf_kernel<1>, dim3((n_images + 63) / 64), dim3(64), 0, s, n_images, res_y, (const void*)d_cdf_y, d_cdf_y, d_img_total, (float*)nullptr);
	NRS_LAUNCH_CHECK("error_map_cdf_kernel<1> launch");
	hipLaunchKernelGGL(error_map_cdf_kernel<2>, dim3(1), dim3(64), 0, s, 1u, n_images, (const void*)d_img_total, d_cdf_img, (float*)nullptr, d_pmf_img);
	NRS_LAUNCH_CHECK("error_map_cdf_kernel<2> launch");
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
