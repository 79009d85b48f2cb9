// nrs_display.hip -- the streaming kernels between the render kernel's frame and the caller's picture (gfx950): HBM-bound, one thread per pixel.
//
//   accumulate_*         CudaRenderBuffer::accumulate: the running mean over the spp frames of a view.
//   tonemap_*            CudaRenderBuffer::tonemap: the display step after accumulate, with 8-bit output.
//   detile_kernel        multi-GPU tile scatter.
#include <hip/hip_runtime.h>
#include "../../include/nrs.h"
#include "nrs_internal.h"
#include "nrs_launch.h"
#include "nrs_display.h"

namespace nrs {

// ---- CudaRenderBuffer::accumulate (render_buffer.cu:540-560, accumulate_kernel :217-254): the running mean over the spp frames of a view ----------------------
// One thread per pixel, 16 B read x 2 + 16 B written: HBM-bound (100 MB per 1080p frame).  Linear / VisPosNeg are plain fp32 in the reference's order (bit-exact);
// SRGB goes through powf (the device library's here, CUDA's in the reference, glibc's in the oracle: tolerance, not bits).
// one sample joins the running mean of a pixel (accumulate_kernel's body, :217-254)
__device__ __forceinline__ void accumulate_one(float4 color, float4& tmp, float sample_count, int color_space) {
	if (color_space == 2) { // VisPosNeg
		const float val = color.x - color.y;
		float tmp_val = tmp.x - tmp.y;
		tmp_val = (tmp_val * sample_count + val) / (sample_count + 1);
		tmp.x = fmaxf(tmp_val, 0.0f);
		tmp.y = fmaxf(-tmp_val, 0.0f);
	} else {
		if (color_space == 1) { // linear_to_srgb, common_device.cuh:55-61
			color.x = color.x < 0.0031308f ? 12.92f * color.x : 1.055f * powf(color.x, 0.41666f) - 0.055f;
			color.y = color.y < 0.0031308f ? 12.92f * color.y : 1.055f * powf(color.y, 0.41666f) - 0.055f;
			color.z = color.z < 0.0031308f ? 12.92f * color.z : 1.055f * powf(color.z, 0.41666f) - 0.055f;
		}
		tmp.x = (tmp.x * sample_count + color.x) / (sample_count + 1);
		tmp.y = (tmp.y * sample_count + color.y) / (sample_count + 1);
		tmp.z = (tmp.z * sample_count + color.z) / (sample_count + 1);
	}
	tmp.w = (tmp.w * sample_count + color.w) / (sample_count + 1);
}
__global__ __launch_bounds__(256) void accumulate_kernel(uint32_t n, const float4* __restrict__ frame, float4* __restrict__ accum, float sample_count, int color_space, int clear) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	float4 color = frame[i];
	float4 tmp = clear ? make_float4(0.f, 0.f, 0.f, 0.f) : accum[i]; // (sample_count == 0: the reference clears the buffer first, :545-547)
	accumulate_one(color, tmp, sample_count, color_space);
	accum[i] = tmp;
}
// The K slabs of a batch (nrs_render_nerf_spp) folded into the running mean in sample order: the per-sample update above K times in registers -- the running mean is not
// associative, so no sum-then-divide -- with one read and one write of the accumulate buffer instead of K.  Every intermediate is the fp32 value K launches of
// accumulate_kernel would have stored and read back: bit-equal to them.
__global__ __launch_bounds__(256) void accumulate_spp_kernel(uint32_t n, const float4* __restrict__ frames, size_t slab_stride, uint32_t spp_count, float4* __restrict__ accum,
                                                             uint32_t sample_count, int color_space) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	float4 tmp = sample_count == 0u ? make_float4(0.f, 0.f, 0.f, 0.f) : accum[i];
	float4 color = frames[i];
	for (uint32_t k = 0; k < spp_count; ++k) {
		const float4 next = k + 1u < spp_count ? frames[(size_t)(k + 1u) * slab_stride + i] : color; // (the next slab's load is in flight during this sample's divisions)
		accumulate_one(color, tmp, (float)(sample_count + k), color_space);
		color = next;
	}
	accum[i] = tmp;
}
int launch_accumulate(uint32_t n_pixels, const float* d_frame, float* d_accum, uint32_t sample_count, int color_space, void* stream) {
	if (n_pixels == 0) return NRS_OK;
	hipLaunchKernelGGL(accumulate_kernel, dim3((n_pixels + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_pixels, reinterpret_cast<const float4*>(d_frame),
	                   reinterpret_cast<float4*>(d_accum), (float)sample_count, color_space, sample_count == 0 ? 1 : 0);
	NRS_LAUNCH_CHECK("accumulate_kernel launch");
	return NRS_OK;
}
int launch_accumulate_spp(uint32_t n_pixels, const float* d_frames, size_t slab_stride_pixels, uint32_t spp_count, float* d_accum, uint32_t sample_count, int color_space, void* stream) {
	if (n_pixels == 0 || spp_count == 0) return NRS_OK;
	hipLaunchKernelGGL(accumulate_spp_kernel, dim3((n_pixels + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_pixels, reinterpret_cast<const float4*>(d_frames), slab_stride_pixels,
	                   spp_count, reinterpret_cast<float4*>(d_accum), sample_count, color_space);
	NRS_LAUNCH_CHECK("accumulate_spp_kernel launch");
	return NRS_OK;
}

// ---- CudaRenderBuffer::tonemap (render_buffer.cu:562-580, tonemap_kernel :471-501, tonemap :254-332): the display step after accumulate ----------------------------
// One thread per pixel, lanes on consecutive pixels: a wave loads 1 KiB contiguous and stores 1 KiB (RGBA32F) or 256 B (RGBA8) contiguous.  HBM-bound like accumulate
// (32 or 20 B per pixel).  Everything is plain fp32 in the reference's operation order (-ffp-contract=off, no fmaf: bit-exact against a float restatement) except the two
// powf of the sRGB curves (the device library's: tolerance, as in accumulate_kernel).  These are the reference's curves (common_device.cuh:31-37, :55-61) with their powf and
// their division -- not nrs_shade.cuh's srgb_to_linear, whose exp2/log2 form is good to 1e-5 only, enough for a network's colour but not for this step's 2e-6.
__device__ __forceinline__ float tonemap_srgb_to_linear(float s) { return s <= 0.04045f ? s / 12.92f : powf((s + 0.055f) / 1.055f, 2.4f); }
__device__ __forceinline__ float tonemap_linear_to_srgb(float l) { return l < 0.0031308f ? 12.92f * l : 1.055f * powf(l, 0.41666f) - 0.055f; }
// Array3f::cwiseMax(0.f) / cwiseMin(1.f) as Eigen evaluates them: (a < b) ? b : a and (b < a) ? b : a -- a NaN and the sign of a zero pass through
__device__ __forceinline__ float tonemap_max0(float x) { return x < 0.0f ? 0.0f : x; }
__device__ __forceinline__ float tonemap_min1(float x) { return 1.0f < x ? 1.0f : x; }
// tonemap(Array3f x, ETonemapCurve) of one channel for the two rational curves, :304-308
__device__ __forceinline__ float tonemap_rational(float x, float k0, float k1, float k2, float k3, float k4, float k5) {
	const float sq = x * x;
	const float nom = (sq * k0 + k1 * x) + k2;
	const float denom = (k3 * sq + k4 * x) + k5;
	return nom / denom;
}
// What is uniform across the frame: scale = 2^exposure and, for a colour space other than SRGB, the background's srgb_to_linear (tonemap_kernel does both in every
// thread, :483-485, :321), are evaluated once by launch_tonemap on the host.
struct TonemapArgs {
	float scale;        // powf(2.0f, exposure)
	float bg[4];        // background colour in the accumulate buffer's space
	int color_space;    // EColorSpace of the accumulate buffer
	int out_space;      // EColorSpace of the output (Linear | SRGB)
	int curve;          // ETonemapCurve
	int clamp;          // clamp_output_color
};
// tonemap_kernel's per-pixel work (:487-495) on the value of the accumulate buffer; the branches are wave-uniform
__device__ __forceinline__ float4 tonemap_pixel(float4 c, const TonemapArgs& t) {
	const float weight = (1 - c.w) * t.bg[3];
	c.x += t.bg[0] * weight;
	c.y += t.bg[1] * weight;
	c.z += t.bg[2] * weight;
	c.w += weight;
	if (t.color_space == 1) { c.x = tonemap_srgb_to_linear(c.x); c.y = tonemap_srgb_to_linear(c.y); c.z = tonemap_srgb_to_linear(c.z); } // 1. to linear (VisPosNeg is linear red / green)
	c.x *= t.scale; c.y *= t.scale; c.z *= t.scale;                                                                                 // 2. exposure
	if (t.curve != 0) {                                                                                                               // 3. the curve; Identity returns x untouched
		c.x = tonemap_max0(c.x); c.y = tonemap_max0(c.y); c.z = tonemap_max0(c.z);
		if (t.curve == 3) { // Reinhard
			const float Y = (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z;
			const float s = 1.f / (Y + 1.0f);
			c.x *= s; c.y *= s; c.z *= s;
		} else {
			float k0, k1, k2, k3, k4, k5; // constants: folded at compile time, in IEEE fp32 and in this order
			if (t.curve == 1) { // ACES, pre-exposure 0.6 inside the coefficients
				k0 = 0.6f * 0.6f * 2.51f; k1 = 0.6f * 0.03f; k2 = 0.0f;
				k3 = 0.6f * 0.6f * 2.43f; k4 = 0.6f * 0.59f; k5 = 0.14f;
			} else { // Hable, white point 11.2 and exposure bias 2 inside the coefficients
				const float A = 0.15f, B = 0.50f, C = 0.10f, D = 0.20f, E = 0.02f, F = 0.30f, W = 11.2f;
				k0 = A * F - A * E; k1 = C * B * F - B * E; k2 = 0.0f;
				k3 = A * F; k4 = B * F; k5 = D * F * F;
				const float nom = k0 * (W * W) + k1 * W + k2;
				const float denom = k3 * (W * W) + k4 * W + k5;
				const float white_scale = denom / nom;
				k0 = 4.0f * k0 * white_scale; k1 = 2.0f * k1 * white_scale; k2 = k2 * white_scale;
				k3 = 4.0f * k3; k4 = 2.0f * k4;
			}
			c.x = tonemap_rational(c.x, k0, k1, k2, k3, k4, k5);
			c.y = tonemap_rational(c.y, k0, k1, k2, k3, k4, k5);
			c.z = tonemap_rational(c.z, k0, k1, k2, k3, k4, k5);
		}
	}
	if (t.out_space == 1) { c.x = tonemap_linear_to_srgb(c.x); c.y = tonemap_linear_to_srgb(c.y); c.z = tonemap_linear_to_srgb(c.z); } // 4. to the output's space
	if (t.clamp) {
		c.x = tonemap_min1(tonemap_max0(c.x)); c.y = tonemap_min1(tonemap_max0(c.y));
		c.z = tonemap_min1(tonemap_max0(c.z)); c.w = tonemap_min1(tonemap_max0(c.w));
	}
	return c;
}
// RGBA32F: the float4 the reference writes to its surface and to lopi.  RGBA8: one dword, bytes R, G, B, A in memory; the clamp is implied (fmaxf / fminf: a NaN becomes 0).
template <int FMT>
__device__ __forceinline__ void tonemap_store(void* out, uint32_t i, float4 c) {
	if (FMT == NRS_TONEMAP_RGBA32F) {
		reinterpret_cast<float4*>(out)[i] = c;
	} else {
		const uint32_t r = (uint32_t)(fminf(fmaxf(c.x, 0.0f), 1.0f) * 255.0f + 0.5f), g = (uint32_t)(fminf(fmaxf(c.y, 0.0f), 1.0f) * 255.0f + 0.5f);
		const uint32_t b = (uint32_t)(fminf(fmaxf(c.z, 0.0f), 1.0f) * 255.0f + 0.5f), a = (uint32_t)(fminf(fmaxf(c.w, 0.0f), 1.0f) * 255.0f + 0.5f);
		reinterpret_cast<uint32_t*>(out)[i] = r | (g << 8) | (b << 16) | (a << 24);
	}
}
// `out` may be `accum` itself for RGBA32F (no __restrict__ on either): a lane reads its pixel before it writes it and touches no other.
template <int FMT>
__global__ __launch_bounds__(256) void tonemap_kernel(uint32_t n, const float4* accum, const TonemapArgs t, void* out) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	tonemap_store<FMT>(out, i, tonemap_pixel(accum[i], t));
}
// accumulate_spp_kernel's fold, then tonemap_pixel on the value it stores: the last batch of a view and its display step in one pass (K slabs read, the accumulate buffer
// read once and written once, the output written once).  The same device functions as the two kernels it replaces: bit-equal to them.  `out` aliases nothing here.
template <int FMT>
__global__ __launch_bounds__(256) void accumulate_spp_tonemap_kernel(uint32_t n, const float4* __restrict__ frames, size_t slab_stride, uint32_t spp_count, float4* __restrict__ accum,
                                                                     uint32_t sample_count, const TonemapArgs t, void* __restrict__ out) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	float4 tmp = sample_count == 0u ? make_float4(0.f, 0.f, 0.f, 0.f) : accum[i];
	float4 color = frames[i];
	for (uint32_t k = 0; k < spp_count; ++k) {
		const float4 next = k + 1u < spp_count ? frames[(size_t)(k + 1u) * slab_stride + i] : color;
		accumulate_one(color, tmp, (float)(sample_count + k), t.color_space);
		color = next;
	}
	accum[i] = tmp;
	tonemap_store<FMT>(out, i, tonemap_pixel(tmp, t));
}
static TonemapArgs tonemap_args(const nrs_tonemap_params& p) {
	TonemapArgs t;
	t.scale = powf(2.0f, p.exposure);
	for (int c = 0; c < 4; ++c) t.bg[c] = p.background_color[c];
	if (p.color_space != NRS_COLOR_SRGB) // the background is sRGB-encoded: to linear unless that is the space the buffer is in (:483-485)
		for (int c = 0; c < 3; ++c) t.bg[c] = t.bg[c] <= 0.04045f ? t.bg[c] / 12.92f : powf((t.bg[c] + 0.055f) / 1.055f, 2.4f);
	t.color_space = (int)p.color_space; t.out_space = (int)p.output_color_space; t.curve = (int)p.tonemap_curve; t.clamp = (int)p.clamp_output;
	return t;
}
int launch_tonemap(uint32_t n_pixels, const float* d_accum, const nrs_tonemap_params& p, void* d_out, void* stream) {
	if (n_pixels == 0) return NRS_OK;
	const TonemapArgs t = tonemap_args(p);
	const dim3 grid((n_pixels + 255) / 256), block(256);
	if (p.output_format == NRS_TONEMAP_RGBA8) hipLaunchKernelGGL(tonemap_kernel<NRS_TONEMAP_RGBA8>, grid, block, 0, (hipStream_t)stream, n_pixels, reinterpret_cast<const float4*>(d_accum), t, d_out);
	else hipLaunchKernelGGL(tonemap_kernel<NRS_TONEMAP_RGBA32F>, grid, block, 0, (hipStream_t)stream, n_pixels, reinterpret_cast<const float4*>(d_accum), t, d_out);
	NRS_LAUNCH_CHECK("tonemap_kernel launch");
	return NRS_OK;
}
int launch_accumulate_spp_tonemap(uint32_t n_pixels, const float* d_frames, size_t slab_stride_pixels, uint32_t spp_count, float* d_accum, uint32_t sample_count,
                                  const nrs_tonemap_params& p, void* d_out, void* stream) {
	if (n_pixels == 0 || spp_count == 0) return NRS_OK;
	const TonemapArgs t = tonemap_args(p);
	const dim3 grid((n_pixels + 255) / 256), block(256);
	if (p.output_format == NRS_TONEMAP_RGBA8)
		hipLaunchKernelGGL(accumulate_spp_tonemap_kernel<NRS_TONEMAP_RGBA8>, grid, block, 0, (hipStream_t)stream, n_pixels, reinterpret_cast<const float4*>(d_frames), slab_stride_pixels,
		                   spp_count, reinterpret_cast<float4*>(d_accum), sample_count, t, d_out);
	else
		hipLaunchKernelGGL(accumulate_spp_tonemap_kernel<NRS_TONEMAP_RGBA32F>, grid, block, 0, (hipStream_t)stream, n_pixels, reinterpret_cast<const float4*>(d_frames), slab_stride_pixels,
		                   spp_count, reinterpret_cast<float4*>(d_accum), sample_count, t, d_out);
	NRS_LAUNCH_CHECK("accumulate_spp_tonemap_kernel launch");
	return NRS_OK;
}

// ---- multi-GPU de-tiling ---------------------------------------------------------------------------------------------------
__global__ void detile_kernel(int W, int H, uint32_t tile, uint32_t tiles_x, uint32_t n_ranks, size_t rank_stride, const float* __restrict__ tiles,
                              uint32_t channels, float* __restrict__ image) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= (uint32_t)(W * H)) return;
	const uint32_t x = i % (uint32_t)W, y = i / (uint32_t)W;
	const uint32_t T = (y / tile) * tiles_x + (x / tile);
	const uint32_t r = T % n_ranks, k = T / n_ranks;
	const size_t src = (size_t)r * rank_stride + ((((size_t)k * tile + (y % tile)) * tile + (x % tile))) * channels;
	for (uint32_t c = 0; c < channels; ++c) image[(size_t)i * channels + c] = tiles[src + c];
}

int launch_detile(const nrs_render_params& p, uint32_t n_ranks, size_t rank_stride_floats, const float* d_tiles, uint32_t channels,
                  float* d_image, void* stream) {
	const int W = p.resolution[0], H = p.resolution[1];
	const uint32_t tiles_x = tile_pitch((uint32_t)W, p.tile_size);
	const uint32_t n = (uint32_t)(W * H);
	hipLaunchKernelGGL(detile_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, W, H, p.tile_size, tiles_x, n_ranks, rank_stride_floats,
	                   d_tiles, channels, d_image);
	NRS_LAUNCH_CHECK("detile_kernel launch");
	return NRS_OK;
}

} // namespace nrs
