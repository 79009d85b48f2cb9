// nrs_metrics.hip -- image metrics on the device (gfx950, wave64): PSNR's squared error and run.py's SSIM of a rendered view against a reference image
// (include/nrs.h, "image metrics"; the arithmetic: nrs_metrics.h).
//
//   image_metrics_kernel<REF_FMT>   a workgroup of 256 threads owns a 32 x 32 tile of pixels: stencil (5 x 5 separable blur of five quantities) and reduce.
//   image_metrics_finish_kernel     one thread: n_pixels, mse, ssim, psnr from the two sums.
#include <hip/hip_runtime.h>
#include "../../include/nrs.h"
#include "nrs_launch.h"
#include "nrs_metrics.h"

namespace nrs {

// The tile: kTile x kTile output pixels, read with the blur's halo as kIn x kIn = 36 x 36 pixels of both images (1.27 x the tile), each pixel loaded ONCE.
//   phase 1  every thread loads pixels of the haloed tile (16 B of the image, 8 or 16 B of the reference; lanes on consecutive pixels of a 36-pixel row), forms
//            La and Lb into LDS, and -- where the pixel is one of the tile's own -- its three squared errors, summed in fixed point in a register.  Halo coordinates go
//            through the reflect rule on the IMAGE's axes: every address is inside the image, whatever the tile's position and the image's size (1 x 1 included).
//   phase 2  the five quantities (La, Lb, La^2, Lb^2, La Lb) blurred along y into LDS: kTile rows x kIn columns each.
//   phase 3  along x into registers, four pixels per thread (lanes on consecutive pixels of a row), the pixel's ssim, summed in fixed point.
//   phase 4  the two sums through the wave (shuffles) and the workgroup (LDS); thread 0 issues one no-return 64-bit integer atomic per sum.
// LDS: 2 x 36 x 36 x 4 B + 5 x 32 x 36 x 4 B + 64 B = 33 472 B -> four workgroups per CU.
constexpr int kTile = 32, kIn = kTile + 2 * kMetricsHalo, kThreads = 256;
static_assert(kTile * kTile % kThreads == 0, "phase 3 gives every thread the same number of pixels");

struct MetricsArgs {
	int width, height;
	const float4* image;
	const void* reference;
	MetricsPixelArgs px;
	nrs_image_metrics_result* result;
	float* ssim_map;    // nullable
	float* sq_err_map;  // nullable
};

template <int REF_FMT>
__device__ __forceinline__ void metrics_load_reference(const void* reference, size_t p, float rf[4]) {
	if (REF_FMT == NRS_IMAGE_RGBA16F_LINEAR) {
		const uint2 h = reinterpret_cast<const uint2*>(reference)[p];
		rf[0] = metrics_half_to_float((uint16_t)(h.x & 0xffffu)); rf[1] = metrics_half_to_float((uint16_t)(h.x >> 16));
		rf[2] = metrics_half_to_float((uint16_t)(h.y & 0xffffu)); rf[3] = metrics_half_to_float((uint16_t)(h.y >> 16));
	} else {
		const float4 v = reinterpret_cast<const float4*>(reference)[p];
		rf[0] = v.x; rf[1] = v.y; rf[2] = v.z; rf[3] = v.w;
	}
}

template <int REF_FMT>
__global__ __launch_bounds__(kThreads) void image_metrics_kernel(const MetricsArgs a) {
	__shared__ float s_la[kIn * kIn], s_lb[kIn * kIn];
	__shared__ float s_y[5][kTile * kIn];
	__shared__ long long s_red[2][kThreads / 64];
	const int tid = (int)threadIdx.x;
	const int x0 = (int)blockIdx.x * kTile, y0 = (int)blockIdx.y * kTile;
	long long sum_sq = 0, sum_ssim = 0;

	for (int i = tid; i < kIn * kIn; i += kThreads) { // phase 1
		const int ly = i / kIn, lx = i - ly * kIn;
		const int ux = x0 + lx - kMetricsHalo, uy = y0 + ly - kMetricsHalo; // may lie outside the image
		const int gx = metrics_reflect(ux, a.width), gy = metrics_reflect(uy, a.height);
		const size_t p = (size_t)gy * (size_t)a.width + (size_t)gx;
		const float4 c = a.image[p];
		const float img[3] = {c.x, c.y, c.z};
		float rf[4];
		metrics_load_reference<REF_FMT>(a.reference, p, rf);
		const MetricsPixel px = metrics_pixel(img, rf, a.px);
		s_la[i] = px.la;
		s_lb[i] = px.lb;
		const bool own = lx >= kMetricsHalo && lx < kMetricsHalo + kTile && ly >= kMetricsHalo && ly < kMetricsHalo + kTile && ux < a.width && uy < a.height;
		if (own) { // (ux, uy) == (gx, gy) here
			sum_sq += (metrics_fixed(px.e[0]) + metrics_fixed(px.e[1])) + metrics_fixed(px.e[2]);
			if (a.sq_err_map) a.sq_err_map[p] = metrics_sq_err_mean(px);
		}
	}
	__syncthreads();

	for (int o = tid; o < kTile * kIn; o += kThreads) { // phase 2: output row oy of the tile reads rows oy .. oy + 4 of the haloed tile
		const int oy = o / kIn, ox = o - oy * kIn;
		float la[5], lb[5];
		for (int k = 0; k < 5; ++k) {
			la[k] = s_la[(oy + k) * kIn + ox];
			lb[k] = s_lb[(oy + k) * kIn + ox];
		}
		s_y[0][o] = metrics_blur5(la[0], la[1], la[2], la[3], la[4]);
		s_y[1][o] = metrics_blur5(lb[0], lb[1], lb[2], lb[3], lb[4]);
		s_y[2][o] = metrics_blur5(la[0] * la[0], la[1] * la[1], la[2] * la[2], la[3] * la[3], la[4] * la[4]);
		s_y[3][o] = metrics_blur5(lb[0] * lb[0], lb[1] * lb[1], lb[2] * lb[2], lb[3] * lb[3], lb[4] * lb[4]);
		s_y[4][o] = metrics_blur5(la[0] * lb[0], la[1] * lb[1], la[2] * lb[2], la[3] * lb[3], la[4] * lb[4]);
	}
	__syncthreads();

	for (int o = tid; o < kTile * kTile; o += kThreads) { // phase 3: output column px of the tile reads columns px .. px + 4
		const int py = o / kTile, px = o - py * kTile;
		const int gx = x0 + px, gy = y0 + py;
		if (gx < a.width && gy < a.height) {
			float v[5];
			for (int q = 0; q < 5; ++q) {
				const float* row = &s_y[q][py * kIn + px];
				v[q] = metrics_blur5(row[0], row[1], row[2], row[3], row[4]);
			}
			const float s = metrics_ssim(v[0], v[1], v[2], v[3], v[4]);
			sum_ssim += metrics_fixed(s);
			if (a.ssim_map) a.ssim_map[(size_t)gy * (size_t)a.width + (size_t)gx] = s;
		}
	}

	for (int d = 32; d > 0; d >>= 1) { // phase 4
		sum_sq += __shfl_down(sum_sq, d);
		sum_ssim += __shfl_down(sum_ssim, d);
	}
	if ((tid & 63) == 0) {
		s_red[0][tid >> 6] = sum_sq;
		s_red[1][tid >> 6] = sum_ssim;
	}
	__syncthreads();
	if (tid == 0) {
		long long t0 = 0, t1 = 0;
		for (int w = 0; w < kThreads / 64; ++w) {
			t0 += s_red[0][w];
			t1 += s_red[1][w];
		}
		(void)__hip_atomic_fetch_add((long long*)&a.result->sum_sq_err, t0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		(void)__hip_atomic_fetch_add((long long*)&a.result->sum_ssim, t1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
}

__global__ void image_metrics_finish_kernel(nrs_image_metrics_result* result, uint32_t n_pixels) { metrics_finish(result, n_pixels); }

int launch_image_metrics(uint32_t width, uint32_t height, const float* d_image, const void* d_reference, int reference_format, const MetricsPixelArgs& px,
                         nrs_image_metrics_result* d_result, float* d_ssim_map, float* d_sq_err_map, void* stream) {
	hipStream_t s = (hipStream_t)stream;
	hipError_t e = hipMemsetAsync(d_result, 0, 16, s); // the two sums
	if (e != hipSuccess) return hip_fail(e, "image metrics: clearing the sums");
	MetricsArgs a{};
	a.width = (int)width; a.height = (int)height;
	a.image = reinterpret_cast<const float4*>(d_image); a.reference = d_reference; a.px = px;
	a.result = d_result; a.ssim_map = d_ssim_map; a.sq_err_map = d_sq_err_map;
	const dim3 grid((width + kTile - 1) / kTile, (height + kTile - 1) / kTile), block(kThreads);
	if (reference_format == NRS_IMAGE_RGBA16F_LINEAR) hipLaunchKernelGGL(image_metrics_kernel<NRS_IMAGE_RGBA16F_LINEAR>, grid, block, 0, s, a);
	else hipLaunchKernelGGL(image_metrics_kernel<NRS_IMAGE_RGBA32F_LINEAR>, grid, block, 0, s, a);
	NRS_LAUNCH_CHECK("image_metrics_kernel launch");
	hipLaunchKernelGGL(image_metrics_finish_kernel, dim3(1), dim3(1), 0, s, d_result, width * height);
	NRS_LAUNCH_CHECK("image_metrics_finish_kernel launch");
	return NRS_OK;
}

} // namespace nrs
