// nrs_camera.cuh -- primary rays: the lens models, the distortion map and the environment map, pixel_to_ray and the ray a pixel starts with.
// Citations as in nrs_grid_math.cuh.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/nrs.h"
#include "nrs_internal.h"
#include "nrs_vec.cuh"
#include "nrs_grid_math.cuh"
#include "nrs_random.cuh"

namespace nrs {

// ---- primary rays: pixel_to_ray (common_device.cuh:245-295) + init_rays_with_payload_kernel_nerf (tn:2512-2616) -------
struct Ray { f3 o, d; float t; bool alive; };

// square2disk_shirley, random_val.cuh:109-125.  sincosf is the device library's (<= 2 ulp): the thin-lens branch is the one place on the path where
// ray origins are not bit-identical to the host-compiled reference (glibc's sincosf) -- nor is CUDA's; tests/test_gpu_modes.py states the tolerance.
__device__ __forceinline__ void square2disk_shirley(float a, float b, float& ox, float& oy) {
	const float PI = 3.14159265358979323846f;
	float phi, r;
	if (a * a > b * b) { r = a; phi = (PI / 4.0f) * (b / a); }
	else { r = b; phi = (PI / 2.0f) - (PI / 4.0f) * (a / b); }
	float sin_phi, cos_phi;
	sincosf(phi, &sin_phi, &cos_phi);
	ox = r * cos_phi; oy = r * sin_phi;
}

// ---- camera model and background (LENS instantiations only) ------------------------------------------------------------------------------------
// apply_camera_distortion / iterative_camera_undistortion (common_device.cuh:146-200): OpenCV radial + tangential model, undone by Newton iterations with
// a central-difference Jacobian and Eigen's 2x2 inverse (adjugate times 1 / det) -- plain fp32 in the reference's order: bit-identical to the oracle.
__device__ __forceinline__ void apply_camera_distortion(const float* prm, float u, float v, float& du, float& dv) {
	const float k1 = prm[0], k2 = prm[1], p1 = prm[2], p2 = prm[3];
	const float u2 = u * u, uv = u * v, v2 = v * v, r2 = u2 + v2;
	const float radial = k1 * r2 + k2 * r2 * r2;
	du = u * radial + 2.f * p1 * uv + p2 * (r2 + 2.f * u2);
	dv = v * radial + 2.f * p2 * uv + p1 * (r2 + 2.f * v2);
}
__device__ __forceinline__ void iterative_camera_undistortion(const float* prm, float& u, float& v) {
	const float kMaxStepNorm = 1e-10f, kRelStepSize = 1e-6f, eps = 1.1920928955078125e-07f;
	const float x00 = u, x01 = v;
	float x0 = u, x1 = v;
	#pragma unroll 1
	for (uint32_t i = 0; i < 100; ++i) {
		const float step0 = fmaxf(eps, fabsf(kRelStepSize * x0)), step1 = fmaxf(eps, fabsf(kRelStepSize * x1));
		float dx0, dx1, b00, b01, f00, f01, b10, b11, f10, f11;
		apply_camera_distortion(prm, x0, x1, dx0, dx1);
		apply_camera_distortion(prm, x0 - step0, x1, b00, b01);
		apply_camera_distortion(prm, x0 + step0, x1, f00, f01);
		apply_camera_distortion(prm, x0, x1 - step1, b10, b11);
		apply_camera_distortion(prm, x0, x1 + step1, f10, f11);
		const float J00 = 1 + (f00 - b00) / (2 * step0), J01 = (f10 - b10) / (2 * step1), J10 = (f01 - b01) / (2 * step0), J11 = 1 + (f11 - b11) / (2 * step1);
		const float invdet = 1.0f / (J00 * J11 - J10 * J01);
		const float i00 = J11 * invdet, i10 = -J10 * invdet, i01 = -J01 * invdet, i11 = J00 * invdet;
		const float r0 = x0 + dx0 - x00, r1 = x1 + dx1 - x01;
		const float s0 = i00 * r0 + i01 * r1, s1 = i10 * r0 + i11 * r1;
		x0 -= s0; x1 -= s1;
		if (s0 * s0 + s1 * s1 < kMaxStepNorm) break;
	}
	u = x0; v = x1;
}
// f_theta_undistortion (common_device.cuh:231-243): the direction through (uvx, uvy) of an f-theta lens with screen centre (cx, cy) -- the params are r0..r4, width, height --
// into `dir`; false where the reference returns its error direction (the caller's: the render path and the dataset's rays name different ones), `dir` untouched.
template <typename P>
__device__ __forceinline__ bool f_theta_undistortion(P prm, float uvx, float uvy, float cx, float cy, f3& dir) {
	const float xpix = (uvx - cx) * prm[5], ypix = (uvy - cy) * prm[6];
	const float norm = sqrtf(xpix * xpix + ypix * ypix);
	const float alpha = prm[0] + norm * (prm[1] + norm * (prm[2] + norm * (prm[3] + norm * prm[4])));
	float sin_alpha, cos_alpha;
	sincosf(alpha, &sin_alpha, &cos_alpha);
	if (cos_alpha <= 1.17549435e-38f || norm == 0.f) return false;
	sin_alpha *= 1.f / norm;
	dir = {sin_alpha * xpix, sin_alpha * ypix, cos_alpha};
	return true;
}
// read_image<2> (common_device.cuh:80-110): bilinear, texels clamped
__device__ __forceinline__ void read_image2(const float* __restrict__ data, const int32_t* res, float px, float py, float& o0, float& o1) {
	const float fx = px * (float)(res[0] - 1), fy = py * (float)(res[1] - 1);
	const int tx = (int)fx, ty = (int)fy;
	const float wx = fx - (float)tx, wy = fy - (float)ty;
	const int x0 = max(min(tx, res[0] - 1), 0), x1 = max(min(tx + 1, res[0] - 1), 0), y0 = max(min(ty, res[1] - 1), 0), y1 = max(min(ty + 1, res[1] - 1), 0);
	const float2* d = reinterpret_cast<const float2*>(data);
	const float2 a = d[x0 + y0 * res[0]], b = d[x1 + y0 * res[0]], c = d[x0 + y1 * res[0]], e = d[x1 + y1 * res[0]];
	const float w00 = (1 - wx) * (1 - wy), w10 = (wx) * (1 - wy), w01 = (1 - wx) * (wy), w11 = (wx) * (wy);
	o0 = ((w00 * a.x + w10 * b.x) + w01 * c.x) + w11 * e.x;
	o1 = ((w00 * a.y + w10 * b.y) + w01 * c.y) + w11 * e.y;
}
// read_envmap (envmap.cuh:30-63): spherical coordinates of the direction (acosf / atan2f: the device library's, as sincosf in the thin-lens branch --
// tolerance, not bits, against the host-compiled reference), bilinear lookup wrapping in x and clamped in y
// Its two halves, each stated once: the footprint of a direction -- the texel and the bilinear weights, before wrapping and clamping -- and the lookup at a footprint.
// The render path calls them back to back (read_envmap); the training path keeps the footprint between the background and the envmap's gradient (nrs_envmap.hip).
struct EnvmapFootprint { int tx, ty; float wx, wy; };
__device__ __forceinline__ EnvmapFootprint envmap_footprint(const int32_t* res, f3 dir) {
	const float PI = 3.14159265358979323846f;
	const f3 d = {dir.z, -dir.x, dir.y};
	const float theta = acosf(fminf(fmaxf(d.z, -1.0f), 1.0f));
	const float phi = atan2f(d.y, d.x);
	const float cyl_x = theta / PI, cyl_y = (phi / (2.0f * PI) + 0.5f);
	const float fx = cyl_y * (float)(res[0] - 1), fy = cyl_x * (float)(res[1] - 1);
	const int tx = (int)fx, ty = (int)fy;
	return EnvmapFootprint{tx, ty, fx - (float)tx, fy - (float)ty};
}
__device__ __forceinline__ float4 envmap_lookup(const float* __restrict__ data, const int32_t* res, const EnvmapFootprint& f) {
	const int tx = f.tx, ty = f.ty;
	const float wx = f.wx, wy = f.wy;
	auto wrapx = [&](int x) { return x < 0 ? x + res[0] : (x >= res[0] ? x - res[0] : x); };
	const int x0 = wrapx(tx), x1 = wrapx(tx + 1), y0 = max(min(ty, res[1] - 1), 0), y1 = max(min(ty + 1, res[1] - 1), 0);
	const float4* q = reinterpret_cast<const float4*>(data);
	const float4 a = q[x0 + y0 * res[0]], b = q[x1 + y0 * res[0]], c = q[x0 + y1 * res[0]], e = q[x1 + y1 * res[0]];
	const float w00 = (1 - wx) * (1 - wy), w10 = (wx) * (1 - wy), w01 = (1 - wx) * (wy), w11 = (wx) * (wy);
	return make_float4(((w00 * a.x + w10 * b.x) + w01 * c.x) + w11 * e.x, ((w00 * a.y + w10 * b.y) + w01 * c.y) + w11 * e.y,
	                   ((w00 * a.z + w10 * b.z) + w01 * c.z) + w11 * e.z, ((w00 * a.w + w10 * b.w) + w01 * c.w) + w11 * e.w);
}
__device__ __forceinline__ float4 read_envmap(const float* __restrict__ data, const int32_t* res, f3 dir) { return envmap_lookup(data, res, envmap_footprint(res, dir)); }

// pixel_to_ray (common_device.cuh:245-295): origin and UN-normalised direction of pixel (x, y) through the camera of its ray time
// (init_rays_with_payload_kernel_nerf, tn:2551-2567).  offset = ld_random_pixel_offset(snap ? 0 : spp), computed once per thread by the caller.
// LENS compiles in the thin-lens branch (:285-293; m_dof, focus distance focus_z = plane_z): only the instantiations that serve dof != 0 carry it.
// SPP: the Sobol sample index is the argument `spp`, not p.spp_index (a batch of samples of one view in one launch, nrs_render_nerf_spp: the index differs per packet)
//      and, where `vw` is given, the two cameras, the focal length and the aperture are that sample's own (nrs_render_nerf_spp_views): the same arithmetic on the
//      record's floats as on the params' -- the same bits as a single frame whose params hold them.  The record is read through a pointer with an explicit address
//      space, never through one that could be merged with a pointer into the params: the kernel arguments would then be copied to scratch for every launch.
//      UNIFORM: `vw` is the same in every lane (the fill: one packet, one sample) -- the record is constant for the life of the kernel and comes in through scalar loads.
template <bool LENS = false, bool SPP = false, bool UNIFORM = false>
__device__ __forceinline__ void pixel_ray_raw(const nrs_render_params& p, uint32_t x, uint32_t y, float off_x, float off_y, float focus_z, f3& o, f3& d, bool use_dof = true, uint32_t spp = 0u,
                                              const nrs_sample_view* vw = nullptr) {
	const float W = (float)p.resolution[0], H = (float)p.resolution[1];
	const uint32_t idx = x + (uint32_t)p.resolution[0] * y;
	float u = ((float)x + 0.5f) * (1.f / W);
	float v = ((float)y + 0.5f) * (1.f / H);
	float ray_time = p.rolling_shutter[0] + p.rolling_shutter[1] * u + p.rolling_shutter[2] * v;
	float rs_rand = (p.rolling_shutter[3] != 0.f) ? ld_random_val(SPP ? spp : p.spp_index, idx * 72239731u) : 0.f; // x * 0 == 0 for finite x
	ray_time = ray_time + p.rolling_shutter[3] * rs_rand;
	float cam[12], v_focal_x = 0.f, v_focal_y = 0.f, v_dof = 0.f; // (v_*: the view's; without a view every use below reads the params where it always did)
	const bool viewed = SPP && vw;
	if (!viewed) {
		#pragma unroll
		for (int i = 0; i < 12; ++i) cam[i] = p.camera_matrix0[i] * ray_time + p.camera_matrix1[i] * (1.f - ray_time);
	} else { // (the focal length and the aperture now; the cameras where they are used, below)
		if (UNIFORM) {
			const NRS_CONSTANT float* c = (const NRS_CONSTANT float*)vw;
			v_focal_x = c[24]; v_focal_y = c[25]; v_dof = c[26];
			if (use_dof) focus_z = c[27];
		} else {
			const NRS_GLOBAL float* c = (const NRS_GLOBAL float*)vw;
			v_focal_x = c[24]; v_focal_y = c[25]; v_dof = c[26];
			if (use_dof) focus_z = c[27];
		}
	}
	float uvx = ((float)x + off_x) / W;
	float uvy = ((float)y + off_y) / H;
	f3 dir = {(uvx - p.screen_center[0]) * W / (viewed ? v_focal_x : p.focal_length[0]), (uvy - p.screen_center[1]) * H / (viewed ? v_focal_y : p.focal_length[1]), 1.0f};
	if (LENS && p.distortion_mode == 2u) { // FTheta, :263-267
		if (!f_theta_undistortion(p.distortion_params, uvx, uvy, p.screen_center[0], p.screen_center[1], dir)) { // the error direction: a point outside the aabb so that the pixel is not rendered
			o = mk3(1000.f, 0.f, 0.f); d = mk3(0.f, 0.f, 1.f);
			return;
		}
	} else if (LENS && p.distortion_mode == 1u) {
		iterative_camera_undistortion(p.distortion_params, dir.x, dir.y);
	}
	if (LENS && p.d_distortion_map) { // :278-280
		float d0, d1;
		read_image2(p.d_distortion_map, p.distortion_resolution, uvx, uvy, d0, d1);
		dir.x += d0; dir.y += d1;
	}
	if (viewed) { // the view's cameras, read HERE and not above the lens code: cam[] would live through it in vector registers (the params' are re-read from the kernel arguments)
		static_assert(offsetof(nrs_sample_view, camera_matrix1) == 48 && offsetof(nrs_sample_view, focal_length) == 96 && offsetof(nrs_sample_view, slice_plane_z) == 108, "record layout");
		if (UNIFORM) {
			const NRS_CONSTANT float* c = (const NRS_CONSTANT float*)vw;
			#pragma unroll
			for (int i = 0; i < 12; ++i) cam[i] = c[i] * ray_time + c[12 + i] * (1.f - ray_time);
		} else {
			const NRS_GLOBAL float* c = (const NRS_GLOBAL float*)vw;
			#pragma unroll
			for (int i = 0; i < 12; ++i) cam[i] = c[i] * ray_time + c[12 + i] * (1.f - ray_time);
		}
	}
	d = mat3_mul(cam, dir); // camera_matrix.block<3, 3>(0, 0) * dir, common_device.cuh:282
	o = {cam[9], cam[10], cam[11]};
	if (LENS && use_dof && (viewed ? v_dof : p.dof) != 0.0f) {
		const f3 lookat = o + d * focus_z;
		float r0, r1, bx, by;
		ld_random_val_2d(SPP ? spp : p.spp_index, x * 19349663u + y * 96925573u, r0, r1);
		square2disk_shirley(r0 * 2.0f - 1.0f, r1 * 2.0f - 1.0f, bx, by);
		bx = (viewed ? v_dof : p.dof) * bx; by = (viewed ? v_dof : p.dof) * by;
		o = {o.x + (cam[0] * bx + cam[3] * by), o.y + (cam[1] * bx + cam[4] * by), o.z + (cam[2] * bx + cam[5] * by)};
		const f3 diff = lookat - o;
		d = {diff.x / focus_z, diff.y / focus_z, diff.z / focus_z};
	}
}
// origin and normalised direction (tn:2588)
template <bool LENS = false, bool SPP = false, bool UNIFORM = false>
__device__ __forceinline__ void ray_origin_dir(const nrs_render_params& p, uint32_t x, uint32_t y, float off_x, float off_y, f3& o, f3& d, uint32_t spp = 0u, const nrs_sample_view* vw = nullptr) {
	pixel_ray_raw<LENS, SPP, UNIFORM>(p, x, y, off_x, off_y, p.slice_plane_z, o, d, true, spp, vw); // (a view brings its own focus distance)
	float n = sqrtf(dot3(d, d));
	d = {d.x / n, d.y / n, d.z / n};
}

template <bool LENS = false, bool SPP = false>
__device__ __forceinline__ Ray init_ray(const nrs_render_params& p, uint32_t x, uint32_t y, float off_x, float off_y, uint32_t spp = 0u, const nrs_sample_view* vw = nullptr) {
	Ray r;
	ray_origin_dir<LENS, SPP, SPP>(p, x, y, off_x, off_y, r.o, r.d, spp, vw); // (the fill: the packet's sample is wave-uniform)
	float tmin;
	ray_intersect(p.render_aabb_min, p.render_aabb_max, r.o, r.d, tmin);
	r.t = fmaxf(tmin, NRS_NEAR_DISTANCE) + 1e-6f;
	Box3 bb;
	#pragma unroll
	for (int i = 0; i < 3; ++i) { bb.mn[i] = p.render_aabb_min[i]; bb.mx[i] = p.render_aabb_max[i]; }
	r.alive = box_contains(bb, r.o + r.d * r.t);
	return r;
}

} // namespace nrs
