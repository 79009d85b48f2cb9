// nrs_optimizer.hip -- the optimiser step (include/nrs.h "optimiser", DESIGN.md "The optimiser step"): tiny-cuda-nn's Adam with a per-parameter step counter, the
// zero-gradient skip, L2 on the matrix weights, the fp16 copy the network reads, the EMA of that copy and the gradient's reset, in ONE pass over the parameters.
//   adam_step_kernel     four elements per lane: 16-byte accesses on grad / master / m / v / steps / ema, 8 bytes for the four fp16; grid-striding; scalar tail.
//   ema_kernel           the EMA in a launch of its own (measurement variant; the fused form measured faster: profiles/optimizer.md).
//   adam_init_kernel, round_fp16_kernel   nrs_optimizer_set_weights / _export_fp16.
// Memory-bound: 42 B per live element with zero_grad, 4 B per skipped one.  All arithmetic is fp32 without contraction (-ffp-contract=off) in the order nrs.h gives, with
// IEEE division and square root, so the result can be compared against a float32 restatement bit by bit.  The bias correction comes from a host-made table, not from powf.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "../../include/nrs.h"
#include "nrs_launch.h"
#include "nrs_optimizer.h"

namespace nrs {

namespace {

__device__ __forceinline__ uint16_t f32_to_f16_bits(float x) {
	const _Float16 h = (_Float16)x; // v_cvt_f16_f32, round to nearest even
	return __builtin_bit_cast(uint16_t, h);
}
__device__ __forceinline__ float f16_bits_to_f32(uint16_t b) { return (float)__builtin_bit_cast(_Float16, b); }
__device__ __forceinline__ uint16_t* fp16_at(const Fp16Dest& h, uint32_t i) { return i < h.split ? h.h_lo + i : h.h_hi + (i - h.split); }

// One element of the rule.  Returns false for a skipped element (everything left as it was).
__device__ __forceinline__ bool adam_element(const AdamStepArgs& a, const float* __restrict__ table, bool matrix, float graw, float& w, float& m, float& v, uint32_t& t) {
	float g = graw / a.loss_scale;
	if (!matrix && g == 0.0f) return false; // (-0 compares equal)
	if (matrix) g = g + a.l2_reg * w;
	m = a.beta1 * m + a.one_minus_beta1 * g;
	v = a.beta2 * v + a.one_minus_beta2 * (g * g);
	t = t + 1u;
	const float lr = (matrix ? a.lr_matrix : a.lr_other) * table[t < a.t_sat ? t : a.t_sat];
	w = w - (lr / (sqrtf(v) + a.epsilon)) * m;
	return true;
}

// one element with 4-byte accesses: the tail, and nothing else
template <bool kEma>
__device__ void adam_scalar(const AdamStepArgs& a, const float* __restrict__ table, uint32_t i) {
	const float graw = a.grad[i];
	uint16_t* hp = fp16_at(a.h, i);
	const bool matrix = i < a.n_matrix;
	uint16_t hb = 0;
	bool live = false;
	if (matrix || graw != 0.0f) {
		float w = a.master[i], m = a.m[i], v = a.v[i];
		uint32_t t = a.steps[i];
		live = adam_element(a, table, matrix, graw, w, m, v, t);
		if (live) {
			hb = f32_to_f16_bits(w);
			a.master[i] = w; a.m[i] = m; a.v[i] = v; a.steps[i] = t; *hp = hb;
		}
	}
	if (kEma) a.ema[i] = a.ema_a * a.ema[i] + a.ema_b * f16_bits_to_f32(live ? hb : *hp);
	if (a.zero_grad && __float_as_uint(graw) != 0u) a.grad[i] = 0.0f;
}

template <bool kEma, bool kLdsTable>
__global__ __launch_bounds__(256) void adam_step_kernel(const AdamStepArgs a) {
	__shared__ float s_table[kLdsTable ? kAdamTableLds + 1 : 1];
	const float* __restrict__ table = a.table;
	if (kLdsTable) {
		for (uint32_t k = threadIdx.x; k <= a.t_sat; k += 256u) s_table[k] = a.table[k];
		__syncthreads();
		table = s_table;
	}
	const uint32_t n_groups = a.n >> 2;
	const bool grad_vec = ((uintptr_t)a.grad & 15u) == 0u; // the caller's buffer: any 4-byte alignment
	for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < n_groups; q += gridDim.x * 256u) {
		const uint32_t i = q << 2;
		float4 g4;
		if (grad_vec) g4 = *reinterpret_cast<const float4*>(a.grad + i);
		else g4 = make_float4(a.grad[i], a.grad[i + 1], a.grad[i + 2], a.grad[i + 3]);
		const float g[4] = {g4.x, g4.y, g4.z, g4.w};
		const bool any_matrix = i < a.n_matrix;
		const bool any_live = any_matrix || g[0] != 0.0f || g[1] != 0.0f || g[2] != 0.0f || g[3] != 0.0f;
		// the four fp16 of this group in one 8-byte access: not across the split, and aligned (always, for the optimiser's own buffers and a split that is a multiple of 4)
		uint16_t* hp = fp16_at(a.h, i);
		const bool h_vec = (i >= a.h.split || i + 4u <= a.h.split) && ((uintptr_t)hp & 7u) == 0u;
		uint16_t hb[4];
		bool all_live = false;
		if (any_live) {
			float4 w4 = *reinterpret_cast<const float4*>(a.master + i), m4 = *reinterpret_cast<const float4*>(a.m + i), v4 = *reinterpret_cast<const float4*>(a.v + i);
			uint4 t4 = *reinterpret_cast<const uint4*>(a.steps + i);
			float w[4] = {w4.x, w4.y, w4.z, w4.w}, m[4] = {m4.x, m4.y, m4.z, m4.w}, v[4] = {v4.x, v4.y, v4.z, v4.w};
			uint32_t t[4] = {t4.x, t4.y, t4.z, t4.w};
			bool live[4];
#pragma unroll
			for (int j = 0; j < 4; ++j) live[j] = adam_element(a, table, i + (uint32_t)j < a.n_matrix, g[j], w[j], m[j], v[j], t[j]);
			all_live = live[0] && live[1] && live[2] && live[3];
			// a skipped element inside a live vector is written back with the bits that were read
			*reinterpret_cast<float4*>(a.master + i) = make_float4(w[0], w[1], w[2], w[3]);
			*reinterpret_cast<float4*>(a.m + i) = make_float4(m[0], m[1], m[2], m[3]);
			*reinterpret_cast<float4*>(a.v + i) = make_float4(v[0], v[1], v[2], v[3]);
			*reinterpret_cast<uint4*>(a.steps + i) = make_uint4(t[0], t[1], t[2], t[3]);
			if (!all_live || !h_vec) { // the fp16 of the skipped ones: as they are
				if (h_vec) {
					const uint2 old = *reinterpret_cast<const uint2*>(hp);
					hb[0] = (uint16_t)old.x; hb[1] = (uint16_t)(old.x >> 16); hb[2] = (uint16_t)old.y; hb[3] = (uint16_t)(old.y >> 16);
				} else {
#pragma unroll
					for (int j = 0; j < 4; ++j) hb[j] = *fp16_at(a.h, i + (uint32_t)j);
				}
			}
#pragma unroll
			for (int j = 0; j < 4; ++j)
				if (live[j]) hb[j] = f32_to_f16_bits(w[j]);
			if (h_vec) {
				*reinterpret_cast<uint2*>(hp) = make_uint2((uint32_t)hb[0] | ((uint32_t)hb[1] << 16), (uint32_t)hb[2] | ((uint32_t)hb[3] << 16));
			} else {
#pragma unroll
				for (int j = 0; j < 4; ++j)
					if (live[j]) *fp16_at(a.h, i + (uint32_t)j) = hb[j];
			}
		} else if (kEma) {
			if (h_vec) {
				const uint2 old = *reinterpret_cast<const uint2*>(hp);
				hb[0] = (uint16_t)old.x; hb[1] = (uint16_t)(old.x >> 16); hb[2] = (uint16_t)old.y; hb[3] = (uint16_t)(old.y >> 16);
			} else {
#pragma unroll
				for (int j = 0; j < 4; ++j) hb[j] = *fp16_at(a.h, i + (uint32_t)j);
			}
		}
		if (kEma) {
			float4 e = *reinterpret_cast<const float4*>(a.ema + i);
			e.x = a.ema_a * e.x + a.ema_b * f16_bits_to_f32(hb[0]);
			e.y = a.ema_a * e.y + a.ema_b * f16_bits_to_f32(hb[1]);
			e.z = a.ema_a * e.z + a.ema_b * f16_bits_to_f32(hb[2]);
			e.w = a.ema_a * e.w + a.ema_b * f16_bits_to_f32(hb[3]);
			*reinterpret_cast<float4*>(a.ema + i) = e;
		}
		if (a.zero_grad && (__float_as_uint(g[0]) | __float_as_uint(g[1]) | __float_as_uint(g[2]) | __float_as_uint(g[3])) != 0u) {
			if (grad_vec) *reinterpret_cast<float4*>(a.grad + i) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
			else {
#pragma unroll
				for (int j = 0; j < 4; ++j)
					if (__float_as_uint(g[j]) != 0u) a.grad[i + j] = 0.0f;
			}
		}
	}
	// the n % 4 elements behind the last group
	if (blockIdx.x == 0u && threadIdx.x < (a.n & 3u)) adam_scalar<kEma>(a, table, (n_groups << 2) + threadIdx.x);
}

// ema[i] = a ema[i] + b float(fp16[i]), four elements per lane where the fp16 allow it
__global__ __launch_bounds__(256) void ema_kernel(uint32_t n, float* __restrict__ ema, const Fp16Dest h, float ea, float eb) {
	const uint32_t n_groups = n >> 2;
	for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < n_groups; q += gridDim.x * 256u) {
		const uint32_t i = q << 2;
		const uint16_t* hp = fp16_at(h, i);
		uint16_t hb[4];
		if ((i >= h.split || i + 4u <= h.split) && ((uintptr_t)hp & 7u) == 0u) {
			const uint2 old = *reinterpret_cast<const uint2*>(hp);
			hb[0] = (uint16_t)old.x; hb[1] = (uint16_t)(old.x >> 16); hb[2] = (uint16_t)old.y; hb[3] = (uint16_t)(old.y >> 16);
		} else {
#pragma unroll
			for (int j = 0; j < 4; ++j) hb[j] = *fp16_at(h, i + (uint32_t)j);
		}
		float4 e = *reinterpret_cast<const float4*>(ema + i);
		e.x = ea * e.x + eb * f16_bits_to_f32(hb[0]);
		e.y = ea * e.y + eb * f16_bits_to_f32(hb[1]);
		e.z = ea * e.z + eb * f16_bits_to_f32(hb[2]);
		e.w = ea * e.w + eb * f16_bits_to_f32(hb[3]);
		*reinterpret_cast<float4*>(ema + i) = e;
	}
	if (blockIdx.x == 0u && threadIdx.x < (n & 3u)) {
		const uint32_t i = (n_groups << 2) + threadIdx.x;
		ema[i] = ea * ema[i] + eb * f16_bits_to_f32(*fp16_at(h, i));
	}
}

__global__ __launch_bounds__(256) void adam_init_kernel(uint32_t n, const float* __restrict__ master, float* __restrict__ ema, const Fp16Dest h) {
	for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
		const float w = master[i];
		ema[i] = w;
		*fp16_at(h, i) = f32_to_f16_bits(w);
	}
}

__global__ __launch_bounds__(256) void round_fp16_kernel(uint32_t n, const float* __restrict__ in, uint16_t* __restrict__ out) {
	for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) out[i] = f32_to_f16_bits(in[i]);
}

// at most 2 048 workgroups of 256 (8 per CU on 256 CUs), grid-striding; never none (block 0 owns the tail)
inline uint32_t stream_grid(uint32_t items) { return std::min<uint32_t>(std::max<uint32_t>((items + 255u) / 256u, 1u), 2048u); }

} // namespace

int launch_adam_step(const AdamStepArgs& a, void* stream) {
	const hipStream_t s = (hipStream_t)stream;
	const bool ema_fused = a.ema_on && !(a.variant & 1u);
	const bool lds = !(a.variant & 2u) && a.t_sat <= kAdamTableLds; // (a longer table stays in L2)
	const dim3 grid(stream_grid(a.n >> 2)), block(256);
	if (ema_fused) {
		if (lds) hipLaunchKernelGGL((adam_step_kernel<true, true>), grid, block, 0, s, a);
		else hipLaunchKernelGGL((adam_step_kernel<true, false>), grid, block, 0, s, a);
	} else {
		if (lds) hipLaunchKernelGGL((adam_step_kernel<false, true>), grid, block, 0, s, a);
		else hipLaunchKernelGGL((adam_step_kernel<false, false>), grid, block, 0, s, a);
	}
	NRS_LAUNCH_CHECK("adam_step_kernel launch");
	if (a.ema_on && !ema_fused) {
		hipLaunchKernelGGL(ema_kernel, grid, block, 0, s, a.n, a.ema, a.h, a.ema_a, a.ema_b);
		NRS_LAUNCH_CHECK("ema_kernel launch");
	}
	return NRS_OK;
}

int launch_adam_init(uint32_t n, const float* master, float* ema, const Fp16Dest& h, void* stream) {
	hipLaunchKernelGGL(adam_init_kernel, dim3(stream_grid(n)), dim3(256), 0, (hipStream_t)stream, n, master, ema, h);
	NRS_LAUNCH_CHECK("adam_init_kernel launch");
	return NRS_OK;
}

int launch_round_fp16(uint32_t n, const float* in, uint16_t* out, void* stream) {
	hipLaunchKernelGGL(round_fp16_kernel, dim3(stream_grid(n)), dim3(256), 0, (hipStream_t)stream, n, in, out);
	NRS_LAUNCH_CHECK("round_fp16_kernel launch");
	return NRS_OK;
}

} // namespace nrs
