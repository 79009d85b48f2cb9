// nrs_network.hip -- the kernels that run the network outside the render kernel (gfx950, wave64).
//
//   network_kernel       NerfNetwork::inference_mixed_precision / density / hash-grid encode on caller batches.
//   grid_eval_kernel     get_density_on_grid / get_rgba_on_grid.
//   selection_rays_kernel, poisson_fit_kernel   the selection tool's ray shooting, the membrane boundary fit.
//   trace_samples_kernel test hook: the (t, dt) stream of listed pixels.
//   slice_kernel         render mode Slice: one sample per pixel on a plane, in the render kernel's packet geometry (nrs_packets.cuh packet_pixel).
#include <hip/hip_runtime.h>
#include "../../include/nrs.h"
#include "nrs_internal.h"
#include "nrs_route.h"
#include "nrs_launch.h"
#include "nrs_render.h"
#include "nrs_network.h"
#include "nrs_vec.cuh"
#include "nrs_grid_math.cuh"
#include "nrs_random.cuh"
#include "nrs_camera.cuh"
#include "nrs_march.cuh"
#include "nrs_shade.cuh"
#include "nrs_hashgrid.cuh"
#include "nrs_mlp.cuh"
#include "nrs_packets.cuh"

namespace nrs {

// ---- render mode Slice ------------------------------------------------------------------------------------------------
// Testbed::render_nerf's Slice branch (tn:3068-3070, 3109-3162): init_rays_with_payload_kernel_nerf with plane_z < 0 leaves every pixel's ray
// standing on the plane at distance |plane_z| along the view axis (tn:2575-2585: t = -plane_z * |d|, depth buffer = -plane_z, no render-box test);
// generate_nerf_network_inputs_at_current_position (tn:616-622) -> NerfNetwork::inference -> compute_nerf_density (tn:624-635: a = 1 - exp(-sigma / 100),
// premultiplied colour) -> shade_kernel_nerf (srgb_to_linear, alpha-over the frame, NO depth write, tn:2474-2482).  One launch: a wave takes an
// 8x8-pixel packet (the render kernel's packet geometry, whole image or owned tiles), a lane a pixel.
template <int NUM>
__global__ __launch_bounds__(256) void slice_kernel(const DeviceModel m, const RenderArgs a) {
	__shared__ NetSmem sm;
	stage_model_to_lds(m, sm.ml);
	const int lane = threadIdx.x & 63;
	const int g = lane >> 5;
	FeatLds& fl = sm.fl[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)];
	const GridView gv = make_grid_view(m);
	const nrs_render_params& p = a.p;
	const uint32_t nm = NUM == kNumRuntime ? (uint32_t)__builtin_amdgcn_readfirstlane((int)m.numerics) : (uint32_t)NUM;
	float off_x, off_y;
	ld_random_pixel_offset(p.snap_to_pixel_centers ? 0u : p.spp_index, off_x, off_y);
	const uint32_t wave_global = blockIdx.x * (blockDim.x >> 6) + (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t n_waves = gridDim.x * (blockDim.x >> 6);
	uint32_t n_px = 0;
	for (uint32_t pk = wave_global; pk < a.n_packets; pk += n_waves) {
		uint32_t x, y, oi;
		const bool have = packet_pixel<1>(a, pk, lane, x, y, oi);
		f3 wpos = mk3(0, 0, 0), wdir = mk3(0.5f, 0.5f, 0.5f);
		if (have) {
			f3 o, d;
			pixel_ray_raw<true>(p, x, y, off_x, off_y, 1.0f, o, d, false); // lens distortion applies; dof = 0 when plane_z < 0 (tn:2543-2545)
			const float n = sqrtf(dot3(d, d));
			const f3 dir = (1.0f / n) * d;
			const float t = p.slice_plane_z * n; // -plane_z * n, plane_z = -(m_slice_plane_z + m_scale)
			wpos = warp_position(o + dir * t, m.aabb);
			wdir = warp_direction(dir);
			a.depth[oi] = p.slice_plane_z; // tn:2583
			if (a.steps) a.steps[oi] = 0;
			++n_px;
		}
		encode_num<NUM>(nm, gv, m.levels, sm.ml, fl, lane, g, wpos, have);
		const f3 pdir = mk3(xchg32(wdir.x), xchg32(wdir.y), xchg32(wdir.z));
		half8 sh_own, sh_par;
		encode_sh4_2(g, wdir, pdir, sh_own, sh_par);
		// (a network trained with light directions: the frame's light direction for every pixel -- a wave-uniform branch, rgb_mlp's LIGHT)
		const NetRaw raw = wave_network<NUM>(nm, fl, sm.ml.w, lane, sh_own, sh_par, m.rgb_deep ? reinterpret_cast<const half8*>(m.wfrag) : nullptr,
		                                     m.n_extra_dims ? reinterpret_cast<const half8*>(m.wfrag) : nullptr, light_operand(g, m.light01[0], m.light01[1], m.light01[2]));
		if (!have) continue;
		const half2v hd = __builtin_bit_cast(half2v, raw.d), hrg = __builtin_bit_cast(half2v, raw.rg), hb = __builtin_bit_cast(half2v, raw.b);
		const float alpha = clampf_(1.f - __expf(-network_to_density((float)hd[0], m.density_activation) / 100.0f), 0.0f, 1.0f);
		float tr = network_to_rgb((float)hrg[0], m.rgb_activation) * alpha, tg = network_to_rgb((float)hrg[1], m.rgb_activation) * alpha,
		      tb = network_to_rgb((float)hb[0], m.rgb_activation) * alpha;
		if (!p.linear_colors) { tr = srgb_to_linear(tr); tg = srgb_to_linear(tg); tb = srgb_to_linear(tb); }
		float4* fb = reinterpret_cast<float4*>(a.frame) + oi;
		const float4 prev = *fb;
		const float om = 1.0f - alpha;
		*fb = make_float4(tr + prev.x * om, tg + prev.y * om, tb + prev.z * om, alpha + prev.w * om);
	}
	// statistics: one evaluated sample, one initialised and one shaded ray per pixel (trace() is not run: n_hit = n_rays_initialized, tn:3109)
	for (int sh = 32; sh > 0; sh >>= 1) n_px += (uint32_t)__shfl_xor((int)n_px, sh, 64);
	if (lane == 0 && n_px) {
		atomicAdd(&a.counters->n_samples, (unsigned long long)n_px);
		atomicAdd(&a.counters->n_rays_alive, n_px);
		atomicAdd(&a.counters->n_rays_hit, n_px);
	}
}
int launch_slice(const DeviceModel& m, const RenderArgs& a, int n_cus, void* stream) {
	if (a.n_packets == 0) return NRS_OK;
	uint32_t grid = (a.n_packets + 3) / 4;
	const uint32_t cap = (uint32_t)n_cus * 8;
	if (grid > cap) grid = cap;
	if (m.numerics) hipLaunchKernelGGL(slice_kernel<kNumRuntime>, dim3(grid), dim3(256), 0, (hipStream_t)stream, m, a);
	else hipLaunchKernelGGL(slice_kernel<0>, dim3(grid), dim3(256), 0, (hipStream_t)stream, m, a);
	NRS_LAUNCH_CHECK("slice_kernel launch");
	return NRS_OK;
}

// ---- trace_samples ------------------------------------------------------------------------------------------------
// LENS: the camera model nrs_render_nerf's EXTRA instantiation marches with (depth of field, lens distortion, the distortion map) -- the hook must
// emit the samples of the rays the renderer really shoots
template <bool LENS>
__global__ void trace_samples_kernel(const DeviceModel m, const nrs_render_params p, uint32_t n_pixels, const uint32_t* __restrict__ pixel_idx,
                                     uint32_t max_samples, float* __restrict__ t_out, float* __restrict__ dt_out, uint32_t* __restrict__ count_out) {
	__shared__ uint32_t coarse[kMarchLdsWords];
	stage_march_lds(coarse, m.occ.mask);
	__syncthreads();
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= n_pixels) return;
	float off_x, off_y;
	ld_random_pixel_offset(p.snap_to_pixel_centers ? 0u : p.spp_index, off_x, off_y);
	const uint32_t idx = pixel_idx[k], W = (uint32_t)p.resolution[0];
	Ray r = init_ray<LENS>(p, idx % W, idx / W, off_x, off_y);
	uint32_t cnt = 0;
	if (r.alive && first_hit(p, m, coarse, idx, r)) {
		float t = r.t;
		while (cnt < max_samples) {
			f3 pos; float dt;
			if (!march_to_occupied(p, m, coarse, r.o, r.d, t, pos, dt)) break;
			t_out[(size_t)k * max_samples + cnt] = t;
			dt_out[(size_t)k * max_samples + cnt] = dt;
			++cnt;
			t += dt;
		}
	}
	count_out[k] = cnt;
}

int launch_trace_samples(const DeviceModel& m, const nrs_render_params& p, uint32_t n_pixels, const uint32_t* d_pixel_idx, uint32_t max_samples,
                         float* d_t, float* d_dt, uint32_t* d_count, void* stream) {
	if (n_pixels == 0) return NRS_OK;
	const bool lens = p.dof != 0.f || p.distortion_mode != 0u || p.d_distortion_map != nullptr;
	if (lens) hipLaunchKernelGGL(trace_samples_kernel<true>, dim3((n_pixels + 127) / 128), dim3(128), 0, (hipStream_t)stream, m, p, n_pixels, d_pixel_idx, max_samples, d_t, d_dt, d_count);
	else hipLaunchKernelGGL(trace_samples_kernel<false>, dim3((n_pixels + 127) / 128), dim3(128), 0, (hipStream_t)stream, m, p, n_pixels, d_pixel_idx, max_samples, d_t, d_dt, d_count);
	NRS_LAUNCH_CHECK("trace_samples_kernel launch");
	return NRS_OK;
}


// ---- selection rays ------------------------------------------------------------------------------------------------
// GrowingSelection::project_selection_pixels (growing_selection.cu:1832-2035) in one launch: shoot_selection_rays_kernel
// (:1673; the ray of pixel_to_ray with spp 0, direction NOT normalised, start at max(t_enter, 0), up to NERF_STEPS samples
// on occupied cells, no min_mip) -> NerfNetwork::density -> composite_shot_rays (:1768; the first sample REACHED with
// T <= threshold is the answer: its position after the warp / unwarp round trip and its occupancy cell).  The reference
// writes every sample, runs the network on all of them and then composites; here a lane owns a ray, the wave evaluates one
// sample per ray and round, and a ray stops at its answer -- the samples behind it are never needed.
constexpr uint32_t kNerfSteps = 1024; // NERF_STEPS, common_nerf.h:20
struct SelectionArgs {
	nrs_render_params p;
	const int32_t* pixels; // [n][2]
	uint32_t n;
	float threshold;
	float* positions;      // [n][3]
	uint32_t* cells;       // [n]
	uint8_t* found;        // [n]
};
template <int NUM>
__global__ __launch_bounds__(256) void selection_rays_kernel(const DeviceModel m, const SelectionArgs a) {
	__shared__ NetSmem sm;
	stage_model_to_lds(m, sm.ml);
	const uint32_t nm = NUM == kNumRuntime ? (uint32_t)__builtin_amdgcn_readfirstlane((int)m.numerics) : (uint32_t)NUM;
	const int lane = threadIdx.x & 63;
	const int g = lane >> 5;
	FeatLds& fl = sm.fl[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)];
	const GridView gv = make_grid_view(m);
	const nrs_render_params& p = a.p;
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	bool have = i < a.n;
	f3 o = mk3(0, 0, 0), d = mk3(0, 0, 1), idir = mk3(0, 0, 0);
	float t = 0.f, T = 1.f;
	uint32_t j = 0;
	if (have) {
		float off_x, off_y;
		ld_random_pixel_offset(0u, off_x, off_y);
		const float W = (float)p.resolution[0], H = (float)p.resolution[1];
		const float uvx = ((float)a.pixels[2 * i] + off_x) / W, uvy = ((float)a.pixels[2 * i + 1] + off_y) / H;
		const f3 dir = {(uvx - p.screen_center[0]) * W / p.focal_length[0], (uvy - p.screen_center[1]) * H / p.focal_length[1], 1.0f};
		const float* cam = p.camera_matrix1;
		d = mat3_mul(cam, dir);
		o = mk3(cam[9], cam[10], cam[11]);
		idir = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
		float tmin;
		ray_intersect(m.aabb.mn, m.aabb.mx, o, d, tmin);
		t = fmaxf(tmin, 0.0f);
		a.found[i] = 0;
		a.cells[i] = 0;
		a.positions[3 * i] = m.aabb.mn[0] - 1.f; a.positions[3 * i + 1] = m.aabb.mn[1] - 1.f; a.positions[3 * i + 2] = m.aabb.mn[2] - 1.f; // :1826
	}
	while (__any(have)) {
		// next sample of the ray (the walk of :1716-1727 / :1754-1765)
		f3 pos = mk3(0, 0, 0);
		float dt = 0.f;
		if (have) {
			bool at_sample = false;
			while (j < kNerfSteps) {
				pos = o + d * t;
				if (!box_contains(m.aabb, pos)) break;
				dt = calc_dt(t, p.cone_angle_constant);
				const uint32_t mip = (uint32_t)mip_from_dt(dt, pos);
				if (density_grid_occupied_at(pos, m.bitfield, mip)) { at_sample = true; break; }
				t = advance_to_next_voxel(t, p.cone_angle_constant, pos, d, idir, kGrid >> mip, 1.0f / (float)(kGrid >> mip));
			}
			if (!at_sample) have = false; // no further sample: transmittance never fell to the threshold (positions stays at the marker)
		}
		const f3 wpos = have ? warp_position(pos, m.aabb) : mk3(0, 0, 0);
		if (have && T <= a.threshold) { // :1802-1809
			const f3 up = unwarp_position(wpos, m.aabb);
			a.positions[3 * i] = up.x; a.positions[3 * i + 1] = up.y; a.positions[3 * i + 2] = up.z;
			const uint32_t level = (uint32_t)mip_from_pos(up);
			a.cells[i] = level * kGridVol + cascaded_grid_idx_at(up, level);
			a.found[i] = 1;
			have = false;
		}
		if (!__any(have)) break;
		encode_num<NUM>(nm, gv, m.levels, sm.ml, fl, lane, g, wpos, have);
		const uint32_t res_d = wave_density<NUM>(nm, fl, sm.ml.w, lane);
		if (have) {
			const float density = network_to_density((float)__builtin_bit_cast(half2v, res_d)[0], m.density_activation);
			const float alpha = 1.f - __expf(-density * unwarp_dt(warp_dt(dt))); // (the reference reads dt back from the NerfCoordinate)
			T *= (1.f - alpha);
			++j;
			t += dt;
		}
	}
}
int launch_selection_rays(const DeviceModel& m, const nrs_render_params& p, const int32_t* d_pixels, uint32_t n, float threshold,
                          float* d_positions, uint32_t* d_cells, uint8_t* d_found, void* stream) {
	if (n == 0) return NRS_OK;
	SelectionArgs a{};
	a.p = p; a.pixels = d_pixels; a.n = n; a.threshold = threshold; a.positions = d_positions; a.cells = d_cells; a.found = d_found;
	if (m.numerics) hipLaunchKernelGGL(selection_rays_kernel<kNumRuntime>, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, m, a);
	else hipLaunchKernelGGL(selection_rays_kernel<0>, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, m, a);
	NRS_LAUNCH_CHECK("selection_rays_kernel launch");
	return NRS_OK;
}

// ---- membrane boundary values -------------------------------------------------------------------------------------
// The device half of GrowingSelection::compute_poisson_boundary (growing_selection.cu:2220-2348) after the network has run on
// the n_sh samples of every cage vertex: activate_network_output (:2182), filter_empty (:2200, is_inside only), the vertex's
// density (its first sample) and the SH9 fit (project_sh9 summed in sample order, times 4 pi / n_sh; sh_utils.cu:30-69).
// One 64-thread workgroup per vertex; thread c < 27 owns coefficient (k = c % 9, colour = c / 9) and sums it sequentially.
__global__ __launch_bounds__(64) void poisson_fit_kernel(const DeviceModel m, uint32_t n_sh, const float* __restrict__ coords /* [n][7] */,
                                                         const _Float16* __restrict__ net /* [n][16] */, int is_inside, float scale,
                                                         float* __restrict__ density_out, float* __restrict__ sh_out /* [n_verts][27] */) {
	const uint32_t v = blockIdx.x, c = threadIdx.x;
	const size_t base = (size_t)v * n_sh;
	if (c == 0) {
		float density = network_to_density((float)net[base * 16 + 3], m.density_activation);
		if (is_inside) {
			const f3 pos = unwarp_position(mk3(coords[base * 7], coords[base * 7 + 1], coords[base * 7 + 2]), m.aabb);
			if (!density_grid_occupied_at(pos, m.bitfield, (uint32_t)mip_from_pos(pos))) density = 0.0f;
		}
		density_out[v] = density;
	}
	if (c >= 27) return;
	const uint32_t kk = c % 9, col = c / 9;
	float acc = 0.f;
	for (uint32_t i = 0; i < n_sh; ++i) {
		const float* co = coords + (base + i) * 7;
		const f3 d = unwarp_direction(mk3(co[4], co[5], co[6]));
		const float rgb = network_to_rgb((float)net[(base + i) * 16 + col], m.rgb_activation);
		const float x = d.x, y = d.y, z = d.z;
		float term;
		switch (kk) { // prefilter.c's constants, rounded to float as the reference's `float c = 0.282095;` does
			case 0: term = rgb * 0.282095f; break;
			case 1: term = rgb * (0.488603f * y); break;
			case 2: term = rgb * (0.488603f * z); break;
			case 3: term = rgb * (0.488603f * x); break;
			case 4: term = rgb * (1.092548f * x * y); break;
			case 5: term = rgb * (1.092548f * y * z); break;
			case 7: term = rgb * (1.092548f * x * z); break;
			case 6: term = rgb * (0.315392f * (3 * z * z - 1)); break;
			default: term = rgb * (0.546274f * (x * x - y * y)); break;
		}
		acc += term; // (times domega = 1.0f: exact)
	}
	sh_out[(size_t)v * 27 + c] = acc * scale;
}
int launch_poisson_fit(const DeviceModel& m, uint32_t n_verts, uint32_t n_sh, const float* d_coords, const void* d_net, int is_inside, float scale,
                       float* d_density, float* d_sh, void* stream) {
	if (n_verts == 0) return NRS_OK;
	hipLaunchKernelGGL(poisson_fit_kernel, dim3(n_verts), dim3(64), 0, (hipStream_t)stream, m, n_sh, d_coords, (const _Float16*)d_net, is_inside, scale, d_density, d_sh);
	NRS_LAUNCH_CHECK("poisson_fit_kernel launch");
	return NRS_OK;
}

// MODE: a NetOp (nrs_network.h).
// 768-thread workgroups: 12 waves share one LDS copy of the weights (24 KB) next to their 12 feature slabs (48 KB), two workgroups per CU
// = 6 waves/SIMD at <= 80 VGPRs.  (256-thread workgroups, the first shape, put 3 workgroups = 3 waves/SIMD on a CU: the weights' copy
// per workgroup was what filled the LDS.)
constexpr int kNetWaves = 12;
// kNetInputGradient and kNetVisualizeActivation (its `layout` = layer | dim << 8, packed by launch_network) are as restated in oracle/nrs_oracle.cpp -- the
// callers of the render path's Normals / EncodingVis modes and of compute_mesh_vertex_normals (tn:4491).
// LIGHT (kNetInference and kNetVisualizeActivation): a network trained with light directions (DeviceModel::n_extra_dims = 3; rgb_mlp's LIGHT) -- every sample gets DeviceModel::light01, or, with
// ld_light != 0, floats 7..9 of its own record (already warped: the reference's PitchedPtr<NerfCoordinate> with extra_stride).  Its kNetInference serves the third hidden layer
// too (a wave-uniform branch on DeviceModel::rgb_deep).  The instantiations without the flag are what they were before it existed.
template <int MODE, int NUM = 0, bool LIGHT = false>
__global__ __launch_bounds__(64 * kNetWaves, (MODE == kNetInputGradient || MODE == kNetVisualizeActivation || LIGHT) ? 3 : 6) void network_kernel(const DeviceModel m, uint32_t n, const float* __restrict__ in, uint32_t ld_in,
                                                      _Float16* __restrict__ out, uint32_t ld_out, int layout, uint32_t ld_light = 0u) {
	constexpr bool FULL = MODE == kNetInference || MODE == kNetInferenceDeep; // (Deep: the full network with a third rgb hidden layer, DeviceModel::rgb_deep -- base_3layer.json)
	const half8* light_w = LIGHT ? reinterpret_cast<const half8*>(m.wfrag) : nullptr;
	const half8* deep_w = (MODE == kNetInferenceDeep || (LIGHT && m.rgb_deep)) ? reinterpret_cast<const half8*>(m.wfrag) : nullptr;
	__shared__ NetSmemT<kNetWaves> sm;
	stage_model_to_lds(m, sm.ml);
	const int lane = threadIdx.x & 63;
	const int g = lane >> 5, j = lane & 31;
	FeatLds& fl = sm.fl[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)];
	const GridView gv = make_grid_view(m);
	const uint32_t wave_global = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	const uint32_t n_waves = gridDim.x * (blockDim.x >> 6);
	const uint32_t n_tiles = (n + 63) / 64;
	for (uint32_t tile = wave_global; tile < n_tiles; tile += n_waves) {
		const uint32_t s = tile * 64 + lane;
		const bool have = s < n;
		f3 wpos = mk3(0, 0, 0), wdir = mk3(0.5f, 0.5f, 0.5f), wlight = mk3(m.light01[0], m.light01[1], m.light01[2]);
		if (have) {
			const float* c = in + (size_t)s * ld_in;
			wpos = mk3(c[0], c[1], c[2]);
			// (NerfNetworkNoDir never looks at the direction rows: a caller may leave them unset, and 0-weights do not stop a NaN)
			if ((FULL || MODE == kNetVisualizeActivation) && !m.no_dir) wdir = mk3(c[4], c[5], c[6]);
			if (LIGHT && ld_light) wlight = mk3(c[7], c[8], c[9]);
		}
		// the light operands of the lane's own sample and of its partner's (lane ^ 32): block b's comes from the lanes 0..31, as for the SH coefficients
		half8 lb_own = half8{}, lb_par = half8{};
		if (LIGHT) {
			lb_own = light_operand(g, wlight.x, wlight.y, wlight.z);
			lb_par = light_operand(g, xchg32(wlight.x), xchg32(wlight.y), xchg32(wlight.z));
		}
		encode_to_lds<(NUM & 1) != 0>(gv, m.levels, sm.ml, fl, lane, g, wpos, have); // (four levels per round trip measured here: ray-ordered batches +-0, random ones -3.5 %: profiles/r06/ab_net_quads.txt; six waves per SIMD hide the trips)

		if (MODE == kNetInputGradient) {
			const f3 gr = wave_density_input_gradient<NUM>((uint32_t)NUM, fl, sm.ml.w, reinterpret_cast<const half8*>(m.wfrag), gv, m.levels, lane, wpos);
			if (have) {
				float* o = reinterpret_cast<float*>(out) + 3 * (size_t)s;
				o[0] = gr.x; o[1] = gr.y; o[2] = gr.z;
			}
			continue;
		}
		if (MODE == kNetVisualizeActivation) {
			const half8 sh_own = encode_sh4(g, wdir), sh_par = encode_sh4(g, mk3(xchg32(wdir.x), xchg32(wdir.y), xchg32(wdir.z)));
			const float v = wave_visualize_activation<NUM, LIGHT>((uint32_t)NUM, fl, sm.ml.w, lane, (uint32_t)layout & 0xffu, (uint32_t)layout >> 8, sh_own, sh_par,
			                                                    m.rgb_deep ? reinterpret_cast<const half8*>(m.wfrag) : nullptr, light_w, lb_own, lb_par, wlight);
			if (have) reinterpret_cast<float*>(out)[s] = v;
			continue;
		}

		if (MODE == kNetEncode) {
			#pragma unroll 1
			for (int b = 0; b < 2; ++b) {
				const uint32_t sb = tile * 64 + 32 * b + j;
				const int sel = (b != g) ? 1 : 0;
				if (sb < n) {
					#pragma unroll
					for (int it = 0; it < 8; ++it) // level 2*it+g, two features per dword
						reinterpret_cast<uint32_t*>(out)[(size_t)sb * 16 + 2 * it + g] = fl.feat[it][sel][lane];
				}
			}
			continue;
		}

		half8 sh_own, sh_par;
		if (FULL) {
			const f3 pdir = mk3(xchg32(wdir.x), xchg32(wdir.y), xchg32(wdir.z));
			sh_own = encode_sh4(g, wdir);
			sh_par = encode_sh4(g, pdir);
		}
		#pragma unroll 1
		for (int b = 0; b < 2; ++b) {
			const int sel = (b != g) ? 1 : 0;
			const half8 x0 = load_features(fl, lane, sel, 0), x1 = load_features(fl, lane, sel, 1);
			const half8 dout = density_mlp<(NUM & 2) != 0>(sm.ml.w, lane, x0, x1);
			half8 rout = dout;
			if (FULL) rout = rgb_mlp<(NUM & 2) != 0, MODE == kNetInferenceDeep || LIGHT, LIGHT>(sm.ml.w, lane, dout, sel ? sh_par : sh_own, deep_w, light_w, sel ? lb_par : lb_own);
			const uint32_t sb = tile * 64 + 32 * b + j;
			if (sb < n) {
				uint32_t ldo = ld_out; // (opaque per tile: the eight 64-bit row offsets were hoisted out of the tile loop and, in the fp16-accumulator twins, spilled)
				asm volatile("" : "+s"(ldo));
				#pragma unroll
				for (int e = 0; e < 8; ++e) {
					const int row = (e & 3) + 8 * (e >> 2) + 4 * g;
					_Float16 v = rout[e];
					if (FULL && e == 3) v = g ? v : dout[0]; // extract_density (nerf_network_full.h:89-95): row 3 <- density row 0, both on g == 0
					if (layout == NRS_PLANES) out[(size_t)row * ldo + sb] = v;
					else out[(size_t)sb * 16 + row] = v;
				}
			}
		}
	}
}

// one operator's kernels, by DeviceModel::numerics
typedef void (*NetKernel)(const DeviceModel, uint32_t, const float*, uint32_t, _Float16*, uint32_t, int, uint32_t);
template <int MODE, bool LIGHT = false>
static NetKernel net_kernel(uint32_t numerics) {
	static constexpr NetKernel k[4] = {network_kernel<MODE, 0, LIGHT>, network_kernel<MODE, 1, LIGHT>, network_kernel<MODE, 2, LIGHT>, network_kernel<MODE, 3, LIGHT>};
	return k[numerics & 3u];
}
int launch_network(const DeviceModel& m, NetOp op, uint32_t n, const float* d_in, uint32_t ld_in, void* d_out, uint32_t ld_out, int layout,
                   int n_cus, void* stream, bool per_sample_light, uint32_t vis_layer, uint32_t vis_dim) {
	if (n == 0) return NRS_OK;
	if (per_sample_light && (!m.n_extra_dims || ld_in < 10u)) { snprintf(g_launch_err, sizeof(g_launch_err), "launch_network: per-sample light directions need n_extra_dims = 3 and ld_in >= 10"); return NRS_ERR_STATE; }
	const uint32_t ld_light = per_sample_light ? 1u : 0u;
	const uint32_t n_tiles = (n + 63) / 64;
	uint32_t grid = (n_tiles + kNetWaves - 1) / kNetWaves;
	const uint32_t cap = (uint32_t)n_cus * 2; // resident workgroups: the tiles are strided over them
	if (grid > cap) grid = cap;
	const bool light = m.n_extra_dims != 0u; // (a light-trained network has LIGHT twins of the two operators that run the rgb MLP)
	NetKernel k;
	switch (op) {
		case kNetInference:
		case kNetInferenceDeep:
			k = light ? net_kernel<kNetInference, true>(m.numerics) : m.rgb_deep ? net_kernel<kNetInferenceDeep>(m.numerics) : net_kernel<kNetInference>(m.numerics);
			break;
		case kNetVisualizeActivation:
			k = light ? net_kernel<kNetVisualizeActivation, true>(m.numerics) : net_kernel<kNetVisualizeActivation>(m.numerics);
			layout = (int)(vis_layer | (vis_dim << 8)); // (in the kernel parameter it has no other use for)
			break;
		case kNetDensity: k = net_kernel<kNetDensity>(m.numerics); break;
		case kNetInputGradient: k = net_kernel<kNetInputGradient>(m.numerics); break;
		default: k = net_kernel<kNetEncode>(m.numerics); break;
	}
	hipLaunchKernelGGL(k, dim3(grid), dim3(64 * kNetWaves), 0, (hipStream_t)stream, m, n, d_in, ld_in, (_Float16*)d_out, ld_out, layout, ld_light);
	NRS_LAUNCH_CHECK("network_kernel launch");
	return NRS_OK;
}

// ---- the network on a regular grid: Testbed::get_density_on_grid (tn:4538) / get_rgba_on_grid (tn:4588) ------------------------
// MODE (a GridEvalOp) kGridDensity: raw density (row 0 of the density MLP) per grid point, -10000 where the density grid says "empty" (grid_samples_half_to_float,
//         tn:464-481); kGridRgba: premultiplied rgba for a fixed view direction (compute_nerf_density, tn:624-635).  The reference
//         materialises the position array and runs the network in 2^20-point batches; here a lane generates its own point.
struct GridEvalArgs {
	uint32_t res[3];
	float box_mn[3], box_mx[3];  // the box the grid spans (world units)
	float dir01[3];              // kGridRgba: warp_direction(ray_dir)
	const float* density_grid;   // kGridDensity: nullable
	float* out;                  // kGridDensity: float [n]; kGridRgba: float4 [n]
};
template <int MODE, int NUM>
__global__ __launch_bounds__(256) void grid_eval_kernel(const DeviceModel m, const GridEvalArgs a) {
	__shared__ NetSmem sm;
	stage_model_to_lds(m, sm.ml);
	const uint32_t nm = NUM == kNumRuntime ? (uint32_t)__builtin_amdgcn_readfirstlane((int)m.numerics) : (uint32_t)NUM;
	const int lane = threadIdx.x & 63;
	const int g = lane >> 5, j = lane & 31;
	FeatLds& fl = sm.fl[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)];
	const GridView gv = make_grid_view(m);
	const uint32_t wave_global = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	const uint32_t n_waves = gridDim.x * (blockDim.x >> 6);
	const uint32_t n = a.res[0] * a.res[1] * a.res[2];
	const uint32_t n_tiles = (n + 63) / 64;
	const f3 wdir = mk3(a.dir01[0], a.dir01[1], a.dir01[2]);
	for (uint32_t tile = wave_global; tile < n_tiles; tile += n_waves) {
		const uint32_t s = tile * 64 + lane;
		const bool have = s < n;
		f3 pos = mk3(0, 0, 0), wpos = mk3(0, 0, 0);
		if (have) { // generate_grid_samples_nerf_uniform(_dir), tn:406-431
			const uint32_t x = s % a.res[0], y = (s / a.res[0]) % a.res[1], z = s / (a.res[0] * a.res[1]);
			pos = mk3((float)x * (1.f / (float)a.res[0]), (float)y * (1.f / (float)a.res[1]), (float)z * (1.f / (float)a.res[2]));
			pos = mk3(pos.x * (a.box_mx[0] - a.box_mn[0]) + a.box_mn[0], pos.y * (a.box_mx[1] - a.box_mn[1]) + a.box_mn[1],
			          pos.z * (a.box_mx[2] - a.box_mn[2]) + a.box_mn[2]);
			wpos = warp_position(pos, m.aabb);
		}
		encode_num<NUM>(nm, gv, m.levels, sm.ml, fl, lane, g, wpos, have);
		NetRaw raw = {0, 0, 0};
		if (MODE == kGridRgba) {
			const half8 sh = encode_sh4(g, wdir);
			raw = wave_network<NUM>(nm, fl, sm.ml.w, lane, sh, sh, m.rgb_deep ? reinterpret_cast<const half8*>(m.wfrag) : nullptr,
			                        m.n_extra_dims ? reinterpret_cast<const half8*>(m.wfrag) : nullptr, light_operand(g, m.light01[0], m.light01[1], m.light01[2]));
		} else {
			raw.d = wave_density<NUM>(nm, fl, sm.ml.w, lane);
		}
		if (!have) continue;
		const float sigma_raw = (float)__builtin_bit_cast(half2v, raw.d)[0];
		if (MODE == kGridDensity) {
			float v = sigma_raw;
			if (a.density_grid) {
				const f3 upos = unwarp_position(wpos, m.aabb);
				const uint32_t mip = (uint32_t)mip_from_pos(upos);
				if (a.density_grid[cascaded_grid_idx_at(upos, mip) + mip * kGridVol] < 0.01f) v = -10000.f; // NERF_MIN_OPTICAL_THICKNESS
			}
			a.out[s] = v;
		} else {
			const half2v hrg = __builtin_bit_cast(half2v, raw.rg), hb = __builtin_bit_cast(half2v, raw.b);
			const float alpha = clampf_(1.f - __expf(-network_to_density(sigma_raw, m.density_activation) / 100.0f), 0.0f, 1.0f);
			reinterpret_cast<float4*>(a.out)[s] = make_float4(network_to_rgb((float)hrg[0], m.rgb_activation) * alpha, network_to_rgb((float)hrg[1], m.rgb_activation) * alpha,
			                                                   network_to_rgb((float)hb[0], m.rgb_activation) * alpha, alpha);
		}
	}
	(void)j;
}

int launch_grid_eval(const DeviceModel& m, GridEvalOp op, const uint32_t res[3], const float box_mn[3], const float box_mx[3], const float dir01[3],
                     const float* d_density_grid, float* d_out, int n_cus, void* stream) {
	GridEvalArgs a{};
	for (int k = 0; k < 3; ++k) { a.res[k] = res[k]; a.box_mn[k] = box_mn[k]; a.box_mx[k] = box_mx[k]; a.dir01[k] = dir01 ? dir01[k] : 0.5f; }
	a.density_grid = d_density_grid;
	a.out = d_out;
	const uint32_t n = res[0] * res[1] * res[2];
	if (n == 0) return NRS_OK;
	const uint32_t n_tiles = (n + 63) / 64;
	uint32_t grid = (n_tiles + 3) / 4; // 256-thread workgroups: 4 waves, a tile each per trip
	const uint32_t cap = (uint32_t)n_cus * 8; // resident workgroups: the tiles are strided over them
	if (grid > cap) grid = cap;
	static constexpr void (*kernels[2][2])(const DeviceModel, const GridEvalArgs) = { // [op][numerics != 0]
		{grid_eval_kernel<kGridDensity, 0>, grid_eval_kernel<kGridDensity, kNumRuntime>}, {grid_eval_kernel<kGridRgba, 0>, grid_eval_kernel<kGridRgba, kNumRuntime>}};
	hipLaunchKernelGGL(kernels[op == kGridDensity ? 0 : 1][m.numerics ? 1 : 0], dim3(grid), dim3(256), 0, (hipStream_t)stream, m, a);
	NRS_LAUNCH_CHECK("grid_eval_kernel launch");
	return NRS_OK;
}

} // namespace nrs
