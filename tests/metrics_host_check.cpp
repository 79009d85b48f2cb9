// metrics_host_check.cpp -- a stand-alone host program (no Python, no HIP, no libnrs.so) over the CPU twin of the image metrics, image_metrics_host of
// nerfshop_amd/csrc/nrs_metrics.h: what nrs_image_metrics_host runs.  tests/test_metrics_host.py builds it with the host compiler under
// -fsanitize=address,undefined and runs it on the CPU: a 37 x 53 image (no multiple of anything, both axes longer than the blur), both reference formats, both
// colour spaces, with maps, then 1 x 1 and 2 x 3 (axes shorter than the blur's reach).  It prints one line per case; the test compares the sums with the library's.
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tests/metrics_host_check.cpp -o metrics_host_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../nerfshop_amd/csrc/nrs_metrics.h"

// the generator the test repeats: x <- x * 1664525 + 1013904223 (mod 2^32), value = (x >> 8) / 2^24 in [0, 1)
static uint32_t g_state = 12345u;
static float next_unit() {
	g_state = g_state * 1664525u + 1013904223u;
	return (float)(g_state >> 8) * (1.0f / 16777216.0f);
}
// a float32 in [0, 1) with at most 11 significant bits: exact as an fp16
static uint16_t float_to_half_exact(float f) {
	uint32_t b;
	memcpy(&b, &f, 4);
	if ((b & 0x7fffffffu) == 0) return (uint16_t)(b >> 16);
	const int e = (int)((b >> 23) & 0xffu) - 127 + 15;
	if (e <= 0 || e >= 31 || (b & 0x1fffu)) {
		fprintf(stderr, "float_to_half_exact: %a is not a normal fp16\n", (double)f);
		exit(2);
	}
	return (uint16_t)(((b >> 16) & 0x8000u) | ((uint32_t)e << 10) | ((b >> 13) & 0x3ffu));
}

static int run_case(int width, int height, bool half, int color_space) {
	const size_t n = (size_t)width * height;
	std::vector<float> image(4 * n), ref32(4 * n), ssim_map(n), sq_map(n);
	std::vector<uint16_t> ref16(4 * n);
	for (size_t i = 0; i < 4 * n; ++i) image[i] = next_unit() * 1.25f - 0.125f;                      // some below 0, some above 1
	for (size_t i = 0; i < 4 * n; ++i) ref32[i] = 0.0625f + (float)((int)(next_unit() * 512.0f)) / 1024.0f; // [1/16, 9/16) in steps of 2^-10: exact in fp16
	for (size_t i = 0; i < 4 * n; ++i) ref16[i] = float_to_half_exact(ref32[i]);
	nrs::MetricsPixelArgs px{};
	px.srgb_blend = color_space == NRS_COLOR_SRGB;
	px.bg[0] = 0.25f; px.bg[1] = 0.0f; px.bg[2] = 1.0f;
	nrs_image_metrics_result a{}, b{};
	nrs::image_metrics_host(width, height, image.data(), half ? (const void*)ref16.data() : (const void*)ref32.data(), half, px, &a, ssim_map.data(), sq_map.data());
	nrs::image_metrics_host(width, height, image.data(), half ? (const void*)ref16.data() : (const void*)ref32.data(), half, px, &b, nullptr, nullptr); // NULL maps
	long long from_map = 0;
	for (size_t i = 0; i < n; ++i) from_map += nrs::metrics_fixed(ssim_map[i]);
	const bool ok = a.sum_sq_err == b.sum_sq_err && a.sum_ssim == b.sum_ssim && from_map == (long long)a.sum_ssim && a.n_pixels == n;
	printf("%dx%d %s cs%d sum_sq_err %lld sum_ssim %lld n %u mse %.9g ssim %.9g psnr %.9g %s\n", width, height, half ? "f16" : "f32", color_space, (long long)a.sum_sq_err,
	       (long long)a.sum_ssim, a.n_pixels, (double)a.mse, (double)a.ssim, (double)a.psnr, ok ? "ok" : "MISMATCH");
	return ok ? 0 : 1;
}

int main() {
	int bad = 0;
	const int shapes[3][2] = {{53, 37}, {1, 1}, {3, 2}};
	for (const auto& s : shapes)
		for (int half = 0; half < 2; ++half)
			for (int cs = 0; cs < 2; ++cs) bad += run_case(s[0], s[1], half != 0, cs);
	// an fp16 of every class through the twin's own conversion: zero, subnormal, normal, infinity
	const uint16_t probes[] = {0x0000u, 0x8000u, 0x0001u, 0x03ffu, 0x0400u, 0x3c00u, 0xbc00u, 0x7bffu, 0x7c00u};
	const float want[] = {0.0f, -0.0f, 5.9604644775390625e-8f, 6.09755516052246094e-5f, 6.103515625e-5f, 1.0f, -1.0f, 65504.0f, INFINITY};
	for (int i = 0; i < 9; ++i)
		if (nrs::metrics_half_to_float(probes[i]) != want[i]) { printf("half %04x MISMATCH\n", probes[i]); bad += 1; }
	printf(bad ? "FAILED\n" : "all ok\n");
	return bad ? 1 : 0;
}
