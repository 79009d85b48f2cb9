// nrs_envmap.hip -- the trainable environment map on the device (gfx950, wave64; include/nrs.h, "the environment map").
//
//   envmap_background_kernel        the background a training ray sees (tn:1792-1800): the lookup of the render path (read_envmap's two halves, nrs_camera.cuh) on the
//                                   live texels, composited over the linearised background; the lookup's footprint is kept for the gradient.
//   envmap_accumulate_kernel        the envmap's gradient (tn:1961-1983, deposit_envmap_gradient envmap.cuh:65-101) into signed 64-bit fixed-point cells: no float
//                                   atomic, the sum does not depend on the order of arrival.
//   envmap_cells_to_gradient_kernel the cells as the float gradient the optimiser step reads, and the cells' reset.
// One thread per ray slot; all three are bound by their few memory trips per slot.  fp32 without contraction, in the order nrs.h gives.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "../../include/nrs.h"
#include "nrs_internal.h"
#include "nrs_launch.h"
#include "nrs_envmap.h"
#include "nrs_train.h"
#include "nrs_vec.cuh"
#include "nrs_camera.cuh"
#include "nrs_loss.cuh"
#include "nrs_cells.h"

namespace nrs {

__global__ __launch_bounds__(256) void envmap_background_kernel(const EnvmapBackgroundArgs a) {
	const uint32_t s = blockIdx.x * 256 + threadIdx.x;
	if (s >= live_slots(a.ray_counter, a.n_rays)) return;
	const uint32_t i = a.ray_indices[s];
	if (i >= a.n_rays) return;
	const float* r = a.rays + 6 * (size_t)i;
	const EnvmapFootprint f = envmap_footprint(a.res, mk3(r[3], r[4], r[5]));
	const float4 env = envmap_lookup(a.texels, a.res, f);
	f3 bg = mk3(a.default_background[0], a.default_background[1], a.default_background[2]);
	if (a.background) bg = mk3(a.background[3 * (size_t)s], a.background[3 * (size_t)s + 1], a.background[3 * (size_t)s + 2]);
	const float rest = 1.0f - env.w;
	float* out = a.background_linear + 3 * (size_t)s;
	out[0] = env.x + train_srgb_to_linear(bg.x) * rest;
	out[1] = env.y + train_srgb_to_linear(bg.y) * rest;
	out[2] = env.z + train_srgb_to_linear(bg.z) * rest;
	reinterpret_cast<int4*>(a.footprint)[s] = make_int4(f.tx, f.ty, __float_as_int(f.wx), __float_as_int(f.wy));
}

__global__ __launch_bounds__(256) void envmap_accumulate_kernel(const EnvmapAccumulateArgs a) {
	const uint32_t s = blockIdx.x * 256 + threadIdx.x;
	if (s >= live_slots(a.ray_counter, a.n_rays)) return;
	const uint4* aux = reinterpret_cast<const uint4*>(a.ray_aux + kRayAuxWords * (size_t)s);
	const uint4 a2 = aux[2];
	const uint32_t n = a2.z;
	if (n == 0u || a.numsteps_out[2 * (size_t)s] != n) return; // no samples, stopped, or clipped by the compact buffer (tn:1838, :1961)
	const uint4 a0 = aux[0], a1 = aux[1];
	const float T = __uint_as_float(a0.w);
	float lg[3] = {__uint_as_float(a0.x), __uint_as_float(a0.y), __uint_as_float(a0.z)};
	if (a.envmap_loss_type != a.loss_type) { // tn:1963-1965
		const float target[3] = {__uint_as_float(a1.x), __uint_as_float(a1.y), __uint_as_float(a1.z)};
		const float C[3] = {__uint_as_float(a1.w), __uint_as_float(a2.x), __uint_as_float(a2.y)};
		float loss;
		#pragma unroll
		for (int c = 0; c < 3; ++c) loss_and_gradient(a.envmap_loss_type, target[c], C[c], loss, lg[c]);
	}
	const float scale = a.loss_scale / (float)a.n_rays;
	const float* bl = a.background_linear + 3 * (size_t)s;
	float v[3];
	#pragma unroll
	for (int c = 0; c < 3; ++c) {
		float dbg = T * lg[c];
		if (!a.train_in_linear_colors) dbg = dbg / train_srgb_to_linear_derivative(train_linear_to_srgb(bl[c])); // the loss saw the background sRGB-encoded (tn:1814, :1817)
		v[c] = scale * dbg;
	}
	const int4 f = reinterpret_cast<const int4*>(a.footprint)[s];
	const float wx = __int_as_float(f.z), wy = __int_as_float(f.w);
	// the texels of the lookup: x wraps once and y clamps as envmap_lookup does it; the clamp of x behind the wrap acts for a footprint no lookup wrote alone
	const long long rx = a.res[0], ry = a.res[1];
	auto clamp_to = [](long long x, long long hi) { return x < 0 ? 0ll : (x > hi ? hi : x); };
	auto wrapx = [&](long long x) { return clamp_to(x < 0 ? x + rx : (x >= rx ? x - rx : x), rx - 1); };
	auto clampy = [&](long long y) { return clamp_to(y, ry - 1); };
	const long long x0 = wrapx(f.x), x1 = wrapx((long long)f.x + 1), y0 = clampy(f.y), y1 = clampy((long long)f.y + 1);
	const float w[4] = {(1 - wx) * (1 - wy), wx * (1 - wy), (1 - wx) * wy, wx * wy};
	unsigned long long* const cell[4] = {a.cells + 4 * (x0 + y0 * rx), a.cells + 4 * (x1 + y0 * rx), a.cells + 4 * (x0 + y1 * rx), a.cells + 4 * (x1 + y1 * rx)};
	#pragma unroll
	for (int k = 0; k < 4; ++k) {
		#pragma unroll
		for (int c = 0; c < 3; ++c) signed_cell_deposit(cell[k] + c, v[c] * w[k]); // include/nrs.h, "the environment map", DEPOSIT (alpha's gradient is 0: tn:1981)
	}
}

__global__ __launch_bounds__(256) void envmap_cells_to_gradient_kernel(uint32_t n, unsigned long long* __restrict__ cells, float* __restrict__ grad) {
	for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
		const long long c = (long long)cells[i];
		grad[i] = signed_cell_to_float(c);
		if (c) cells[i] = 0ull;
	}
}

int launch_envmap_background(const EnvmapBackgroundArgs& a, void* stream) {
	if (a.n_rays == 0) return NRS_OK;
	hipLaunchKernelGGL(envmap_background_kernel, dim3((a.n_rays + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
	NRS_LAUNCH_CHECK("envmap_background_kernel launch");
	return NRS_OK;
}
int launch_envmap_accumulate(const EnvmapAccumulateArgs& a, void* stream) {
	if (a.n_rays == 0) return NRS_OK;
	hipLaunchKernelGGL(envmap_accumulate_kernel, dim3((a.n_rays + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
	NRS_LAUNCH_CHECK("envmap_accumulate_kernel launch");
	return NRS_OK;
}
int launch_envmap_cells_to_gradient(uint32_t n, unsigned long long* cells, float* grad, void* stream) {
	const uint32_t grid = std::min<uint32_t>(std::max<uint32_t>((n + 255u) / 256u, 1u), 2048u);
	hipLaunchKernelGGL(envmap_cells_to_gradient_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, n, cells, grad);
	NRS_LAUNCH_CHECK("envmap_cells_to_gradient_kernel launch");
	return NRS_OK;
}

} // namespace nrs
