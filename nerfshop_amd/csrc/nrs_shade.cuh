// nrs_shade.cuh -- what turns network outputs into colour: the activations, sRGB, the glow overlay and the per-sample render modes.
// Citations as in nrs_grid_math.cuh.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/nrs.h"
#include "nrs_internal.h"
#include "nrs_vec.cuh"
#include "nrs_grid_math.cuh"
#include "nrs_random.cuh"

namespace nrs {

// composite_kernel_nerf's glow overlay (tn:806-903; m_glow_mode, off by default): a grid / cut-line visualisation that adds to (or, "grid only", replaces)
// the sample's colour and can scale its weight.  cosf is the device library's (the host-compiled reference uses glibc's): colour tolerance, not bits.
__device__ __forceinline__ void glow_overlay(const nrs_render_params& p, f3 pos, f3 cam_o, float& weight, float& r, float& g, float& b) {
	const uint32_t gm = p.glow_mode;
	const bool green_grid = gm & 1u, green_cutline = gm & 2u, mask_to_alpha = gm & 4u, radial_mode = gm & 8u, grid_mode = gm & 16u;
	float glow = 0.f, dist;
	if (radial_mode) {
		const f3 dv = pos - cam_o;
		dist = sqrtf(dot3(dv, dv));
		dist = fminf(dist, (4.5f - pos.y) * 0.333f);
	} else {
		dist = pos.y;
	}
	if (grid_mode) {
		glow = 1.f / fmaxf(1.f, dist);
	} else {
		float y = p.glow_y_cutoff - dist;
		float mask = 0.f;
		if (y > 0.f) {
			y *= 80.f;
			mask = fminf(1.f, y);
			if (green_cutline) glow += fmaxf(0.f, 1.f - fabsf(1.f - y)) * 4.f;
			if (y > 1.f) y = 1.f - (y - 1.f) * 0.05f;
			if (green_grid) glow += fmaxf(0.f, y / fmaxf(1.f, dist));
		}
		if (mask_to_alpha) weight *= mask;
	}
	if (glow > 0.f) {
		const float PI = 3.141592653589793f;
		float line = 0.f;
		#pragma unroll
		for (int k = 0; k < 4; ++k) { // y, x, z at 2, 4, 8, 16 times the base frequency, in the reference's order
			const float f = (float)(2 << k);
			line += fmaxf(0.f, cosf(pos.y * f * PI * 16.f) - 0.975f);
			line += fmaxf(0.f, cosf(pos.x * f * PI * 16.f) - 0.975f);
			line += fmaxf(0.f, cosf(pos.z * f * PI * 16.f) - 0.975f);
		}
		if (grid_mode) {
			glow = glow * line * 15.f;
			g = glow; b = glow * 0.5f; r = glow * 0.25f;
		} else {
			glow = glow * glow * 0.25f + glow * line * 15.f;
			g += glow; b += glow * 0.5f; r += glow * 0.25f;
		}
	}
}

// composite_kernel_nerf's per-sample render modes (tn:905-937): what replaces the network's colour.  pos = the (mapped) sample position in world
// units, origin = payload.origin, cdt = unwarp_dt(input->dt), alpha after the show_accel override.  Normals / EncodingVis are refused by the host.
__device__ __forceinline__ void render_mode_rgb(const nrs_render_params& p, f3 pos, f3 origin, f3 cam_fwd, float cdt, float alpha, float& r, float& g, float& b) {
	switch (p.render_mode) {
		case NRS_RENDER_POSITIONS:
			if (p.show_accel) { // colour of the occupancy cell the sample stands in (tn:911-920); tcnn::default_rng_t = pcg32(initstate, initseq 1)
				const uint32_t mip = (uint32_t)max((int)p.min_mip, mip_from_pos(pos));
				const float res = (float)(kGrid >> mip);
				const int ix = (int)(pos.x * res), iy = (int)(pos.y * res), iz = (int)(pos.z * res);
				Pcg32 rng{0ull, 3ull};
				rng.next_uint();
				rng.state += (uint64_t)(int64_t)(int)((uint32_t)ix + (uint32_t)iy * 232323u + (uint32_t)iz * 727272u);
				rng.next_uint();
				r = 1.f - (float)mip * (1.f / (float)(kCascades - 1));
				g = rng.next_float();
				b = rng.next_float();
			} else {
				r = (pos.x - 0.5f) / 2.0f + 0.5f; g = (pos.y - 0.5f) / 2.0f + 0.5f; b = (pos.z - 0.5f) / 2.0f + 0.5f;
			}
			break;
		case NRS_RENDER_DEPTH: r = g = b = dot3(cam_fwd, pos - origin) * p.depth_scale; break;
		case NRS_RENDER_DISTANCE: { const f3 dv = pos - origin; r = g = b = sqrtf(dot3(dv, dv)) * p.depth_scale; break; }
		case NRS_RENDER_STEPSIZE: r = g = b = warp_dt(cdt); break;
		case NRS_RENDER_AO: r = g = b = alpha; break;
		default: break; // Shade, Cost: the network's colour
	}
}

// ---- activations (cn:38-66) and shade (common_device.cuh:31-37) ---------------------------------------------------
__device__ __forceinline__ float network_to_rgb(float v, uint32_t act) {
	switch (act) {
		case NRS_ACT_RELU: return v > 0.f ? v : 0.f;
		case NRS_ACT_LOGISTIC: return __builtin_amdgcn_rcpf(1.0f + __expf(-v)); // 1-ulp rcp: inside the stated colour tolerance
		case NRS_ACT_EXPONENTIAL: return __expf(clampf_(v, -10.f, 10.f));
		default: return v;
	}
}
__device__ __forceinline__ float network_to_density(float v, uint32_t act) {
	switch (act) {
		case NRS_ACT_RELU: return v > 0.f ? v : 0.f;
		case NRS_ACT_LOGISTIC: return 1.0f / (1.0f + __expf(-v));
		case NRS_ACT_EXPONENTIAL: return __expf(v);
		default: return v;
	}
}
__device__ __forceinline__ float network_to_density_derivative(float v, uint32_t act) { // tn:308-317
	switch (act) {
		case NRS_ACT_RELU: return v > 0.0f ? 1.0f : 0.0f;
		case NRS_ACT_LOGISTIC: { const float density = 1.0f / (1.0f + __expf(-v)); return density * (1 - density); }
		case NRS_ACT_EXPONENTIAL: return __expf(clampf_(v, -15.0f, 15.0f));
		default: return 1.0f;
	}
}
// x^2.4 as exp2(2.4 * log2 x) on the transcendental unit (v_log_f32 / v_exp_f32, ~1 ulp each): |rel. error| < 1e-5 on
// (0.04, 1], far inside the stated colour tolerance, and ~100 instructions cheaper per channel than powf.
__device__ __forceinline__ float srgb_to_linear(float s) {
	if (s <= 0.04045f) return s * (1.0f / 12.92f);
	return __builtin_amdgcn_exp2f(2.4f * __builtin_amdgcn_logf((s + 0.055f) * (1.0f / 1.055f)));
}

} // namespace nrs
