// nrs_exposure.hip -- per-image exposure on the device (gfx950, wave64; include/nrs.h, "per-image exposure").
//
//   exposure_targets_kernel     the target colour a training ray is compared with (tn:1803-1823): the texel's premultiplied rgb times 2^exposure of its image, gathered
//                               from ray order into slot order in the same pass; the scale is kept for the gradient.
//   exposure_accumulate_kernel  the exposure's gradient (tn:1946-1959) into signed 64-bit fixed-point cells.  A batch touches a handful of images, so one atomic per
//                               lane would queue thousands of adds on three addresses: each wave sums per image in registers first and issues one atomic per image and
//                               channel.  Integer sums: the cells hold the bits one atomic per lane would leave.
//   exposure_step_kernel        adam_optimizer.h's step on every image (tn:3885-3898), the renormalisation (tn:3900-3909) and the cells' reset, in one workgroup.
// fp32 without contraction, in the order nrs.h gives.
#include <hip/hip_runtime.h>
#include "../../include/nrs.h"
#include "nrs_internal.h"
#include "nrs_launch.h"
#include "nrs_exposure.h"
#include "nrs_train.h"
#include "nrs_scan.cuh"
#include "nrs_loss.cuh"
#include "nrs_cells.h"

namespace nrs {

__global__ __launch_bounds__(256) void exposure_targets_kernel(const ExposureTargetsArgs a) {
	const uint32_t s = blockIdx.x * 256 + threadIdx.x;
	if (s >= live_slots(a.ray_counter, a.n_rays)) return;
	const uint32_t i = a.ray_indices[s];
	if (i >= a.n_rays) return;
	const uint32_t img = a.pixels[2 * (size_t)i];
	if (img >= a.n_images) return;
	const float* e = a.exposure + 3 * (size_t)img;
	const float sx = expf(kExposureLn2 * e[0]), sy = expf(kExposureLn2 * e[1]), sz = expf(kExposureLn2 * e[2]);
	const float* t = a.target_rgba + 4 * (size_t)i; // (neither colour array is asked to be 16-byte aligned)
	float* out = a.target_out + 4 * (size_t)s;
	out[0] = sx * t[0]; out[1] = sy * t[1]; out[2] = sz * t[2]; out[3] = t[3];
	reinterpret_cast<uint4*>(a.scale)[s] = make_uint4(__float_as_uint(sx), __float_as_uint(sy), __float_as_uint(sz), img);
}

// Every thread of the workgroup reaches the wave operations below: a slot that deposits nothing carries q = 0 and stays out of the ballots.
__global__ __launch_bounds__(256) void exposure_accumulate_kernel(const ExposureAccumulateArgs a) {
	const uint32_t s = blockIdx.x * 256 + threadIdx.x;
	long long q[3] = {0ll, 0ll, 0ll};
	uint32_t img = 0u;
	if (s < live_slots(a.ray_counter, a.n_rays)) {
		const uint32_t i = a.ray_indices[s];
		if (i < a.n_rays && a.numsteps_out[2 * (size_t)s] > 0u) { // (tn:1838: a ray without compact samples has returned)
			const uint4 sc = reinterpret_cast<const uint4*>(a.scale)[s];
			if (sc.w < a.n_images) {
				img = sc.w;
				const uint4* aux = reinterpret_cast<const uint4*>(a.ray_aux + kRayAuxWords * (size_t)s);
				const uint4 a0 = aux[0], a1 = aux[1];
				const float g[3] = {__uint_as_float(a0.x), __uint_as_float(a0.y), __uint_as_float(a0.z)};
				const float target[3] = {__uint_as_float(a1.x), __uint_as_float(a1.y), __uint_as_float(a1.z)};
				const float scale[3] = {__uint_as_float(sc.x), __uint_as_float(sc.y), __uint_as_float(sc.z)};
				const float pdf = a.xy_pdf ? a.xy_pdf[i] : 1.0f;
				const float per_ray = a.loss_scale / (float)a.n_rays; // tn:1889
				#pragma unroll
				for (int c = 0; c < 3; ++c) {
					float dgt = -g[c] / pdf; // tn:1948
					if (!a.train_in_linear_colors) dgt = dgt / train_srgb_to_linear_derivative(target[c]); // tn:1950-1952
					q[c] = signed_cell_quantise(((per_ray * dgt) * scale[c]) * kExposureLn2); // tn:1955
				}
			}
		}
	}
	const bool deposits = (q[0] | q[1] | q[2]) != 0ll;
#ifdef NRS_EXPOSURE_NO_PEEL // measurements only (tools/exposure_probe.py): one atomic per lane and channel
	if (deposits) {
		#pragma unroll
		for (int c = 0; c < 3; ++c) if (q[c]) cell_add(a.cells + 3 * (size_t)img + c, (unsigned long long)q[c]);
	}
#else
	// peel the wave's distinct images: the first lane left names the image, its lanes are summed across the wave and leave
	const uint32_t lane = threadIdx.x & 63u;
	unsigned long long left = __ballot(deposits);
	while (left) {
		const int first = __builtin_amdgcn_readfirstlane(__ffsll((long long)left) - 1);
		const uint32_t cur = (uint32_t)__builtin_amdgcn_readlane((int)img, first);
		const bool mine = deposits && img == cur;
		long long sum[3];
		#pragma unroll
		for (int c = 0; c < 3; ++c) sum[c] = wave_sum(mine ? q[c] : 0ll);
		// lanes 0..2 add the three channels: one atomic instruction per image and wave, on 24 contiguous bytes
		const long long mine_sum = lane == 0u ? sum[0] : (lane == 1u ? sum[1] : sum[2]);
		if (lane < 3u && mine_sum) cell_add(a.cells + 3 * (size_t)cur + lane, (unsigned long long)mine_sum);
		left &= ~__ballot(mine);
	}
#endif
}

__global__ __launch_bounds__(kExposureMeanLanes) void exposure_step_kernel(const ExposureStepArgs a) {
	__shared__ double s_partial[3][kExposureMeanLanes];
	__shared__ float s_mean[3];
	const uint32_t j = threadIdx.x;
	double partial[3] = {0.0, 0.0, 0.0};
	for (uint32_t i = j; i < a.n_images; i += kExposureMeanLanes) {
		#pragma unroll
		for (int c = 0; c < 3; ++c) {
			const size_t e = 3 * (size_t)i + c;
			float value = a.values[e], m = a.m[e], v = a.v[e];
			const long long cell = (long long)a.cells[e];
			exposure_adam(a.k, cell, value, m, v);
			a.values[e] = value; a.m[e] = m; a.v[e] = v;
			if (cell) a.cells[e] = 0ull;
			partial[c] += (double)value;
		}
	}
	#pragma unroll
	for (int c = 0; c < 3; ++c) s_partial[c][j] = partial[c];
	__syncthreads();
	if (j < 3u) s_mean[j] = exposure_mean(exposure_sum_partials(s_partial[j]), a.n_images);
	__syncthreads();
	const float mean[3] = {s_mean[0], s_mean[1], s_mean[2]};
	for (uint32_t i = j; i < a.n_images; i += kExposureMeanLanes) { // (each thread reads back what it wrote itself)
		#pragma unroll
		for (int c = 0; c < 3; ++c) a.values[3 * (size_t)i + c] -= mean[c];
	}
}

int launch_exposure_targets(const ExposureTargetsArgs& a, void* stream) {
	if (a.n_rays == 0) return NRS_OK;
	hipLaunchKernelGGL(exposure_targets_kernel, dim3((a.n_rays + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
	NRS_LAUNCH_CHECK("exposure_targets_kernel launch");
	return NRS_OK;
}
int launch_exposure_accumulate(const ExposureAccumulateArgs& a, void* stream) {
	if (a.n_rays == 0) return NRS_OK;
	hipLaunchKernelGGL(exposure_accumulate_kernel, dim3((a.n_rays + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
	NRS_LAUNCH_CHECK("exposure_accumulate_kernel launch");
	return NRS_OK;
}
int launch_exposure_step(const ExposureStepArgs& a, void* stream) {
	hipLaunchKernelGGL(exposure_step_kernel, dim3(1), dim3(kExposureMeanLanes), 0, (hipStream_t)stream, a);
	NRS_LAUNCH_CHECK("exposure_step_kernel launch");
	return NRS_OK;
}

} // namespace nrs
