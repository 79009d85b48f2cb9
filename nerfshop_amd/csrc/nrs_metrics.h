// nrs_metrics.h -- image metrics (include/nrs.h, "image metrics"): the per-pixel arithmetic of the definition stated ONCE, for image_metrics_kernel (nrs_metrics.hip)
// and for its CPU twin (image_metrics_host below, behind nrs_image_metrics_host).  Plain C++ with <math.h> only: a host compiler without HIP reads it too
// (tests/metrics_host_check.cpp).  Every expression is float32 in the written order; the translation units that include it are built with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#include "../../include/nrs.h"

#if defined(__HIPCC__)
#define NRS_METRICS_FN __host__ __device__ __forceinline__
#else
#define NRS_METRICS_FN inline
#endif

namespace nrs {

constexpr int kMetricsHalo = 2; // the blur's reach on each side

// run.py's curves (scripts/common.py:139-145) -- not the tonemap's
NRS_METRICS_FN float metrics_linear_to_srgb(float l) { return l > 0.0031308f ? 1.055f * powf(l, 0.41666667f) - 0.055f : 12.92f * l; }
NRS_METRICS_FN float metrics_srgb_to_linear(float s) { return s > 0.04045f ? powf((s + 0.055f) / 1.055f, 2.4f) : s / 12.92f; }
NRS_METRICS_FN float metrics_clip01(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }
NRS_METRICS_FN bool metrics_finite(float x) { return fabsf(x) <= 3.402823466e38f; } // false for a NaN and for an infinity
NRS_METRICS_FN float metrics_luminance(float r, float g, float b) {
	const float e = 0.4545454545f;
	return (0.2126f * powf(r, e) + 0.7152f * powf(g, e)) + 0.0722f * powf(b, e);
}
// scipy's `reflect`: (d c b a | a b c d | d c b a), for every n >= 1 and every i
NRS_METRICS_FN int metrics_reflect(int i, int n) {
	const int m = 2 * n;
	int j = i % m;
	if (j < 0) j += m;
	return j < n ? j : m - 1 - j;
}
// One axis of the blur on v[-2] .. v[2], as the centre plus weighted differences: the centre's weight 0.292082 is 1 - 2 * 0.233881 - 2 * 0.120078 exactly, so this is
// the 5-tap sum with weights that add up to one in float32 as well.  A constant neighbourhood comes back unchanged, bit for bit -- blur(L * L) - blur(L) * blur(L) is then
// exactly 0 there (a flat background, a 1 x 1 image) instead of a few float32 steps of L * L, which the 9e-4 of the SSIM's second factor would magnify to 1e-4.
NRS_METRICS_FN float metrics_blur5(float vm2, float vm1, float v0, float vp1, float vp2) {
	return v0 + (0.233881f * ((vm1 - v0) + (vp1 - v0)) + 0.120078f * ((vm2 - v0) + (vp2 - v0)));
}
// round(v * 2^32) to the nearest integer, ties to even (the product is exact)
NRS_METRICS_FN long long metrics_fixed(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
	return __float2ll_rn(v * 4294967296.0f);
#else
	return llrintf(v * 4294967296.0f);
#endif
}
// an fp16 to float32 (exact)
NRS_METRICS_FN float metrics_half_to_float(uint16_t h) {
#if defined(__HIP_DEVICE_COMPILE__)
	_Float16 v;
	__builtin_memcpy(&v, &h, 2);
	return (float)v;
#else
	const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, exp = (h >> 10) & 0x1fu, man = h & 0x3ffu;
	uint32_t bits;
	if (exp == 0x1fu) bits = sign | 0x7f800000u | (man << 13);
	else if (exp != 0) bits = sign | ((exp + 112u) << 23) | (man << 13);
	else if (man == 0) bits = sign;
	else { // a subnormal half: normalise
		uint32_t m = man, e = 113u;
		while (!(m & 0x400u)) { m <<= 1; e -= 1; }
		bits = sign | (e << 23) | ((m & 0x3ffu) << 13);
	}
	float f;
	memcpy(&f, &bits, 4);
	return f;
#endif
}

// what is uniform across the image
struct MetricsPixelArgs {
	int srgb_blend;  // color_space == NRS_COLOR_SRGB
	float bg[3];
};
// steps 1-4a of one pixel: the rendered rgb and the reference's four floats -> the two luminances and the three squared errors
struct MetricsPixel { float la, lb, e[3]; };
NRS_METRICS_FN MetricsPixel metrics_pixel(const float img[3], const float rf[4], const MetricsPixelArgs& p) {
	float ref[3] = {rf[0], rf[1], rf[2]};
	if (p.srgb_blend) {
		const float a = rf[3];
		for (int c = 0; c < 3; ++c) {
			float v = a != 0.0f ? rf[c] / a : 0.0f;
			v = metrics_linear_to_srgb(v) * a + (1.0f - a) * p.bg[c];
			ref[c] = metrics_srgb_to_linear(v);
		}
	}
	float A[3], R[3];
	MetricsPixel out;
	for (int c = 0; c < 3; ++c) {
		A[c] = metrics_clip01(metrics_linear_to_srgb(img[c]));
		if (!metrics_finite(A[c])) A[c] = 0.0f;
		R[c] = metrics_clip01(metrics_linear_to_srgb(ref[c]));
		const float d = A[c] - R[c];
		const float e = d * d;
		out.e[c] = metrics_finite(e) ? e : 0.0f;
	}
	out.la = metrics_luminance(A[0], A[1], A[2]);
	out.lb = metrics_luminance(R[0], R[1], R[2]);
	return out;
}
NRS_METRICS_FN float metrics_sq_err_mean(const MetricsPixel& px) { return ((px.e[0] + px.e[1]) + px.e[2]) / 3.0f; }
// step 4b: the five blurred quantities of a pixel -> its ssim
NRS_METRICS_FN float metrics_ssim(float mA, float mB, float bAA, float bBB, float bAB) {
	const float sA = bAA - mA * mA, sB = bBB - mB * mB, sAB = bAB - mA * mB;
	const float p1 = (2.0f * mA * mB + 1e-4f) / ((mA * mA + mB * mB) + 1e-4f);
	const float p2 = (2.0f * sAB + 9e-4f) / ((sA + sB) + 9e-4f);
	const float s = p1 * p2;
	return metrics_finite(s) ? s : 0.0f;
}
// step 6: the record from the two sums
NRS_METRICS_FN void metrics_finish(nrs_image_metrics_result* r, uint32_t n_pixels) {
	const double n = (double)n_pixels;
	r->n_pixels = n_pixels;
	r->mse = (float)((double)r->sum_sq_err * (1.0 / 4294967296.0) / (3.0 * n));
	r->ssim = (float)((double)r->sum_ssim * (1.0 / 4294967296.0) / n);
	r->psnr = r->mse == 0.0f ? (float)INFINITY : (float)(-10.0 * log10((double)r->mse));
}

// nrs_metrics.hip: the clear of the two sums, image_metrics_kernel and image_metrics_finish_kernel on `stream`; the arguments have been checked (nrs_api_metrics.cpp)
int launch_image_metrics(uint32_t width, uint32_t height, const float* d_image, const void* d_reference, int reference_format, const MetricsPixelArgs& px,
                         nrs_image_metrics_result* d_result, float* d_ssim_map, float* d_sq_err_map, void* stream);

// The CPU twin: the whole image at once, the arithmetic above.  ref_is_half: the reference is fp16 RGBA (4 x uint16 per pixel), else f32x4.  The maps may be NULL.
inline void image_metrics_host(int width, int height, const float* image, const void* reference, bool ref_is_half, const MetricsPixelArgs& p,
                               nrs_image_metrics_result* result, float* ssim_map, float* sq_err_map) {
	const size_t n = (size_t)width * height;
	std::vector<float> la(n), lb(n), y[5];
	long long sum_sq = 0, sum_ssim = 0;
	for (size_t i = 0; i < n; ++i) {
		float rf[4];
		if (ref_is_half) for (int c = 0; c < 4; ++c) rf[c] = metrics_half_to_float(((const uint16_t*)reference)[4 * i + c]);
		else for (int c = 0; c < 4; ++c) rf[c] = ((const float*)reference)[4 * i + c];
		const MetricsPixel px = metrics_pixel(image + 4 * i, rf, p);
		la[i] = px.la;
		lb[i] = px.lb;
		sum_sq += (metrics_fixed(px.e[0]) + metrics_fixed(px.e[1])) + metrics_fixed(px.e[2]);
		if (sq_err_map) sq_err_map[i] = metrics_sq_err_mean(px);
	}
	for (auto& q : y) q.resize(n);
	for (int r = 0; r < height; ++r) { // along y: La, Lb, La^2, Lb^2, La Lb
		const float *a[5], *b[5];
		for (int k = 0; k < 5; ++k) {
			const size_t row = (size_t)metrics_reflect(r + k - kMetricsHalo, height) * width;
			a[k] = la.data() + row;
			b[k] = lb.data() + row;
		}
		for (int x = 0; x < width; ++x) {
			const size_t o = (size_t)r * width + x;
			y[0][o] = metrics_blur5(a[0][x], a[1][x], a[2][x], a[3][x], a[4][x]);
			y[1][o] = metrics_blur5(b[0][x], b[1][x], b[2][x], b[3][x], b[4][x]);
			y[2][o] = metrics_blur5(a[0][x] * a[0][x], a[1][x] * a[1][x], a[2][x] * a[2][x], a[3][x] * a[3][x], a[4][x] * a[4][x]);
			y[3][o] = metrics_blur5(b[0][x] * b[0][x], b[1][x] * b[1][x], b[2][x] * b[2][x], b[3][x] * b[3][x], b[4][x] * b[4][x]);
			y[4][o] = metrics_blur5(a[0][x] * b[0][x], a[1][x] * b[1][x], a[2][x] * b[2][x], a[3][x] * b[3][x], a[4][x] * b[4][x]);
		}
	}
	for (int r = 0; r < height; ++r) // along x, then the pixel's ssim
		for (int x = 0; x < width; ++x) {
			size_t at[5];
			for (int k = 0; k < 5; ++k) at[k] = (size_t)r * width + metrics_reflect(x + k - kMetricsHalo, width);
			float v[5];
			for (int q = 0; q < 5; ++q) v[q] = metrics_blur5(y[q][at[0]], y[q][at[1]], y[q][at[2]], y[q][at[3]], y[q][at[4]]);
			const float s = metrics_ssim(v[0], v[1], v[2], v[3], v[4]);
			sum_ssim += metrics_fixed(s);
			if (ssim_map) ssim_map[(size_t)r * width + x] = s;
		}
	result->sum_sq_err = sum_sq;
	result->sum_ssim = sum_ssim;
	metrics_finish(result, (uint32_t)n);
}

} // namespace nrs
