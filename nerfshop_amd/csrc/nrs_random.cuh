// nrs_random.cuh -- the two random generators of the device code: the scrambled Sobol sequence (pixel offsets, ray jitter, lens samples)
// and PCG32 (occupancy refresh, training rays).
#pragma once
#include <hip/hip_runtime.h>
#include "nrs_vec.cuh"

namespace nrs {

// ---- scrambled Sobol (random_val.cuh:159-288, 317-322); dims 0 and 1 only ---------------------------------------
// dim 0 direction numbers are 0x80000000 >> bit, i.e. sobol(index, 0) = bit reversal of the index;
// dim 1 obeys v[b] = v[b-1] ^ (v[b-1] >> 1).
__device__ __forceinline__ uint32_t sobol_dim0(uint32_t index) { return __brev(index); }
__device__ __forceinline__ uint32_t sobol_dim1(uint32_t index) {
	uint32_t X = 0, v = 0x80000000u;
	#pragma unroll
	for (uint32_t bit = 0; bit < 32; ++bit) {
		X ^= ((index >> bit) & 1u) ? v : 0u;
		v ^= v >> 1;
	}
	return X;
}
__device__ __forceinline__ uint32_t hash_combine(uint32_t seed, uint32_t v) { return seed ^ (v + (seed << 6) + (seed >> 2)); }
__device__ __forceinline__ uint32_t laine_karras_permutation(uint32_t x, uint32_t seed) {
	x += seed;
	x ^= x * 0x6c50b47cu;
	x ^= x * 0xb82f1e52u;
	x ^= x * 0xc7afe638u;
	x ^= x * 0x8d22f6e6u;
	return x;
}
__device__ __forceinline__ uint32_t nested_uniform_scramble_base2(uint32_t x, uint32_t seed) {
	x = __brev(x);
	x = laine_karras_permutation(x, seed);
	x = __brev(x);
	return x;
}
#define NRS_SOBOL_S 2.3283064365386963e-10f /* float(1.0 / 2^32) */
__device__ __forceinline__ float ld_random_val(uint32_t index, uint32_t seed) { // dim 0
	index = nested_uniform_scramble_base2(index, seed);
	return (float)nested_uniform_scramble_base2(sobol_dim0(index), hash_combine(seed, 0u)) * NRS_SOBOL_S;
}
__device__ __forceinline__ void ld_random_val_2d(uint32_t index, uint32_t seed, float& a, float& b) {
	index = nested_uniform_scramble_base2(index, seed);
	a = (float)nested_uniform_scramble_base2(sobol_dim0(index), hash_combine(seed, 0u)) * NRS_SOBOL_S;
	b = (float)nested_uniform_scramble_base2(sobol_dim1(index), hash_combine(seed, 1u)) * NRS_SOBOL_S;
}
__device__ __forceinline__ void ld_random_pixel_offset(uint32_t spp, float& ox, float& oy) {
	float a0, a1, b0, b1;
	ld_random_val_2d(0u, 0xdeadbeefu, a0, a1);
	ld_random_val_2d(spp, 0xdeadbeefu, b0, b1);
	ox = fractf_((0.5f - a0) + b0);
	oy = fractf_((0.5f - a1) + b1);
}

// tcnn::pcg32 = PCG32 XSH-RR (see oracle/nrs_oracle.cpp for the provenance note); advance() is the LCG skip-ahead.
struct Pcg32 {
	uint64_t state, inc;
	__device__ __forceinline__ uint32_t next_uint() {
		const uint64_t old = state;
		state = old * 0x5851f42d4c957f2dULL + inc;
		const uint32_t xorshifted = (uint32_t)(((old >> 18u) ^ old) >> 27u);
		const uint32_t rot = (uint32_t)(old >> 59u);
		return (xorshifted >> rot) | (xorshifted << ((~rot + 1u) & 31));
	}
	__device__ __forceinline__ float next_float() { return __uint_as_float((next_uint() >> 9) | 0x3f800000u) - 1.0f; }
	// state after `delta` steps = mult * state + plus (mod 2^64)
	__device__ __forceinline__ static void skip_coefficients(uint64_t inc, uint64_t delta, uint64_t& mult, uint64_t& plus) {
		uint64_t cur_mult = 0x5851f42d4c957f2dULL, cur_plus = inc, acc_mult = 1u, acc_plus = 0u;
		while (delta > 0) {
			if (delta & 1) { acc_mult *= cur_mult; acc_plus = acc_plus * cur_mult + cur_plus; }
			cur_plus = (cur_mult + 1) * cur_plus;
			cur_mult *= cur_mult;
			delta >>= 1;
		}
		mult = acc_mult;
		plus = acc_plus;
	}
	__device__ __forceinline__ void advance(uint64_t delta) {
		uint64_t m, p;
		skip_coefficients(inc, delta, m, p);
		state = m * state + p;
	}
};

} // namespace nrs
