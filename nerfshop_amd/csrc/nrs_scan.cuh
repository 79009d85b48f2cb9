// nrs_scan.cuh -- the scans of a wave and of a workgroup, stated once (gfx950, 64 lanes).
//
//   wave_inclusive_add       sum over lanes 0..lane.
//   wave_sum                 sum over the 64 lanes, 64 bits wide (per-image exposure's deposits).
//   wave_segmented_scan      `op` over the lanes st..lane of a segment (seg_scan_mul, seg_scan_add).
//   block_exclusive_add      per-thread values -> "sum in front of this thread" and the workgroup's total, N values at once: the wave scan, then
//   block_combine_waves      the cross-wave half, for a caller that numbers inside its waves itself (mc_count_kernel: ballots).
//
// The three-launch device-wide scans (cage look-up tables, marching cubes, training rays) keep their own tile kernels -- tile size, loads and stores differ -- and share
// these and the one-workgroup scan over the tile sums between them (nrs_scan.hip: launch_tile_scan).  All of it is integer code but wave_segmented_scan, which never
// reassociates: x = op(x, shuffled), under the condition lane >= st + d.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nrs {

__device__ __forceinline__ uint32_t wave_inclusive_add(uint32_t v, uint32_t lane) {
	#pragma unroll
	for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t u = (uint32_t)__shfl_up((int)v, d); if (lane >= d) v += u; }
	return v;
}

// the sum over all 64 lanes, in every lane (a butterfly; integers: no order to keep)
__device__ __forceinline__ long long wave_sum(long long v) {
	#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
	return v;
}

// inclusive scan over the lanes st..lane of a segment (lane >= st)
template <class Op>
__device__ __forceinline__ float wave_segmented_scan(float x, uint32_t lane, uint32_t st, Op op) {
	#pragma unroll
	for (uint32_t d = 1; d < 64; d <<= 1) { const float v = __shfl_up(x, d); if (lane >= st + d) x = op(x, v); }
	return x;
}
// the value one lane up (lane 0: its own)
__device__ __forceinline__ float wave_lane_before(float x) { return __shfl_up(x, 1); }

// wave_total: what the thread's wave sums to, as its last lane holds it.  before = the sum of the waves in front of this thread's, total = of all of them.
// One THREADS / 64 x N array of LDS and one barrier.  Every thread of the workgroup calls it; a kernel that calls it again puts a barrier in between.
template <uint32_t THREADS, uint32_t N>
__device__ __forceinline__ void block_combine_waves(const uint32_t (&wave_total)[N], uint32_t (&before)[N], uint32_t (&total)[N]) {
	__shared__ uint32_t s_wave[THREADS / 64][N];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	if (lane == 63u) {
		#pragma unroll
		for (uint32_t k = 0; k < N; ++k) s_wave[wave][k] = wave_total[k];
	}
	__syncthreads();
	#pragma unroll
	for (uint32_t k = 0; k < N; ++k) before[k] = total[k] = 0u;
	#pragma unroll
	for (uint32_t w = 0; w < THREADS / 64; ++w) {
		#pragma unroll
		for (uint32_t k = 0; k < N; ++k) {
			if (w < wave) before[k] += s_wave[w][k];
			total[k] += s_wave[w][k];
		}
	}
}

// v: this thread's values.  before = the sum of v over the threads in front of this one, total = over the workgroup.
template <uint32_t THREADS, uint32_t N>
__device__ __forceinline__ void block_exclusive_add(const uint32_t (&v)[N], uint32_t (&before)[N], uint32_t (&total)[N]) {
	const uint32_t lane = threadIdx.x & 63u;
	uint32_t inclusive[N];
	#pragma unroll
	for (uint32_t k = 0; k < N; ++k) inclusive[k] = wave_inclusive_add(v[k], lane);
	block_combine_waves<THREADS, N>(inclusive, before, total);
	#pragma unroll
	for (uint32_t k = 0; k < N; ++k) before[k] += inclusive[k] - v[k];
}

} // namespace nrs
