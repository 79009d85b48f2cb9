// nrs_camera.cpp -- the cameras of render_to_cpu's loop on the host: log_space_lerp, CameraKeyframe, the camera path's spline, and the per-sample views of a
// motion-blurred frame (src/python_api.cu:148-158).  No GPU, no context: these load and run without a device, like nrs_tet_lut_build.
// The matrix functions are evaluated in double and rounded once to float ("Unpinned": a restatement of the formulas, not of Eigen's float evaluation).
#include <math.h>
#include <string.h>
#include <string>
#include "../../include/nrs.h"
#include "nrs_internal.h"

using namespace nrs;

namespace {

int cam_fail(int code, const std::string& msg) { set_last_error(msg.c_str()); return code; }

// ---- 4x4 matrices in double, row-major ---------------------------------------------------------------------------------------------------------------
struct M4 { double v[4][4]; };
M4 identity4() { M4 r{}; for (int i = 0; i < 4; ++i) r.v[i][i] = 1.0; return r; }
M4 mul4(const M4& a, const M4& b) {
	M4 r{};
	for (int i = 0; i < 4; ++i)
		for (int j = 0; j < 4; ++j) {
			double s = 0.0;
			for (int k = 0; k < 4; ++k) s += a.v[i][k] * b.v[k][j];
			r.v[i][j] = s;
		}
	return r;
}
M4 add4(const M4& a, const M4& b, double sb = 1.0) { M4 r; for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) r.v[i][j] = a.v[i][j] + sb * b.v[i][j]; return r; }
M4 scale4(const M4& a, double s) { M4 r; for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) r.v[i][j] = a.v[i][j] * s; return r; }
double norm1(const M4& a) { // largest column sum
	double n = 0.0;
	for (int j = 0; j < 4; ++j) { double s = 0.0; for (int i = 0; i < 4; ++i) s += fabs(a.v[i][j]); n = fmax(n, s); }
	return n;
}
// Gauss-Jordan with partial pivoting; false for a (numerically) singular matrix
bool inverse4(const M4& a, M4& out) {
	double w[4][8];
	const double scale = norm1(a);
	for (int i = 0; i < 4; ++i)
		for (int j = 0; j < 4; ++j) { w[i][j] = a.v[i][j]; w[i][4 + j] = i == j ? 1.0 : 0.0; }
	for (int c = 0; c < 4; ++c) {
		int piv = c;
		for (int r = c + 1; r < 4; ++r) if (fabs(w[r][c]) > fabs(w[piv][c])) piv = r;
		if (!(fabs(w[piv][c]) > 1e-14 * scale)) return false;
		if (piv != c) for (int j = 0; j < 8; ++j) { const double t = w[c][j]; w[c][j] = w[piv][j]; w[piv][j] = t; }
		const double inv = 1.0 / w[c][c];
		for (int j = 0; j < 8; ++j) w[c][j] *= inv;
		for (int r = 0; r < 4; ++r) {
			if (r == c) continue;
			const double f = w[r][c];
			if (f != 0.0) for (int j = 0; j < 8; ++j) w[r][j] -= f * w[c][j];
		}
	}
	for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) out.v[i][j] = w[i][4 + j];
	return true;
}
M4 completion(const float m[12]) { // 3x4 column-major -> 4x4 with the row (0, 0, 0, 1)
	M4 r = identity4();
	for (int c = 0; c < 4; ++c) for (int i = 0; i < 3; ++i) r.v[i][c] = (double)m[c * 3 + i];
	return r;
}
// principal square root, Denman-Beavers: Y -> (Y + Z^-1) / 2, Z -> (Z + Y^-1) / 2 from (M, I); false where it does not settle (an eigenvalue on the negative real axis)
bool sqrt4(const M4& m, M4& out) {
	M4 y = m, z = identity4();
	for (int it = 0; it < 60; ++it) {
		M4 yi, zi;
		if (!inverse4(y, yi) || !inverse4(z, zi)) return false;
		const M4 yn = scale4(add4(y, zi), 0.5), zn = scale4(add4(z, yi), 0.5);
		const double step = norm1(add4(yn, y, -1.0)), size = norm1(yn);
		y = yn; z = zn;
		if (!(size < 1e150)) return false;
		if (step <= 4e-16 * size) { out = y; return true; }
	}
	return false;
}
// principal logarithm by inverse scaling and squaring: square roots until X is near I, then log X = 2 atanh((X - I)(X + I)^-1) as its odd series
bool log4(const M4& m, M4& out) {
	M4 x = m;
	int k = 0;
	const M4 one = identity4();
	while (norm1(add4(x, one, -1.0)) > 0.25) {
		if (++k > 48 || !sqrt4(x, x)) return false;
	}
	M4 xp;
	if (!inverse4(add4(x, one), xp)) return false;
	const M4 z = mul4(add4(x, one, -1.0), xp), z2 = mul4(z, z);
	M4 term = z, sum = z;
	for (int n = 3; n <= 41; n += 2) { // |z| <= ~0.15: the terms fall below 1e-17 of the first long before the last
		term = mul4(term, z2);
		sum = add4(sum, term, 1.0 / (double)n);
	}
	out = scale4(sum, 2.0 * ldexp(1.0, k));
	return true;
}
// exponential by scaling and squaring over the Taylor series
M4 exp4(const M4& m) {
	int s = 0;
	double n = norm1(m);
	while (n > 0.5 && s < 64) { n *= 0.5; ++s; }
	const M4 a = scale4(m, ldexp(1.0, -s));
	M4 term = identity4(), sum = identity4();
	for (int k = 1; k <= 20; ++k) {
		term = scale4(mul4(term, a), 1.0 / (double)k);
		sum = add4(sum, term);
	}
	for (int i = 0; i < s; ++i) sum = mul4(sum, sum);
	return sum;
}

// CameraKeyframe::operator* and operator+ (camera_path.h:54-59), float as the reference
nrs_camera_keyframe key_scaled(const nrs_camera_keyframe& k, float f) {
	nrs_camera_keyframe r;
	for (int i = 0; i < 4; ++i) r.R[i] = k.R[i] * f;
	for (int i = 0; i < 3; ++i) r.T[i] = k.T[i] * f;
	r.slice = k.slice * f; r.scale = k.scale * f; r.fov = k.fov * f; r.dof = k.dof * f;
	return r;
}
nrs_camera_keyframe key_sum(const nrs_camera_keyframe& a, const nrs_camera_keyframe& b) {
	float rr[4] = {b.R[0], b.R[1], b.R[2], b.R[3]};
	const float dot = ((rr[0] * a.R[0] + rr[1] * a.R[1]) + rr[2] * a.R[2]) + rr[3] * a.R[3];
	if (dot < 0.f) for (int i = 0; i < 4; ++i) rr[i] = -rr[i];
	nrs_camera_keyframe r;
	for (int i = 0; i < 4; ++i) r.R[i] = a.R[i] + rr[i];
	for (int i = 0; i < 3; ++i) r.T[i] = a.T[i] + b.T[i];
	r.slice = a.slice + b.slice; r.scale = a.scale + b.scale; r.fov = a.fov + b.fov; r.dof = a.dof + b.dof;
	return r;
}
bool finite12(const float* m) { for (int i = 0; i < 12; ++i) if (!std::isfinite(m[i])) return false; return true; }

} // namespace

extern "C" {

// log_space_lerp, src/common_device.cu:27-36
int nrs_log_space_lerp(const float begin[12], const float end[12], float t, float out[12]) {
	if (!begin || !end || !out) return cam_fail(NRS_ERR_INVALID_ARG, "nrs_log_space_lerp: NULL argument");
	if (!finite12(begin) || !finite12(end) || !std::isfinite(t)) return cam_fail(NRS_ERR_INVALID_ARG, "nrs_log_space_lerp: begin, end and t must be finite");
	if (memcmp(begin, end, 12 * sizeof(float)) == 0) { // log(I) = 0: the camera stands still
		memmove(out, begin, 12 * sizeof(float));
		return NRS_OK;
	}
	const M4 a = completion(begin), b = completion(end);
	M4 ai, lg;
	if (!inverse4(a, ai)) return cam_fail(NRS_ERR_INVALID_ARG, "nrs_log_space_lerp: begin is singular");
	if (!log4(mul4(b, ai), lg)) return cam_fail(NRS_ERR_UNSUPPORTED, "nrs_log_space_lerp: end * begin^-1 has no real logarithm within reach (a rotation by 180 degrees, or a singular end)");
	const M4 r = mul4(exp4(scale4(lg, (double)t)), a);
	float res[12];
	for (int c = 0; c < 4; ++c) for (int i = 0; i < 3; ++i) res[c * 3 + i] = (float)r.v[i][c];
	memcpy(out, res, sizeof(res));
	return NRS_OK;
}

// CameraKeyframe::m(), camera_path.h:37-42: Quaternionf(R).normalized().toRotationMatrix() beside T
int nrs_camera_keyframe_matrix(const nrs_camera_keyframe* key, float out[12]) {
	if (!key || !out) return cam_fail(NRS_ERR_INVALID_ARG, "nrs_camera_keyframe_matrix: NULL argument");
	double x = key->R[0], y = key->R[1], z = key->R[2], w = key->R[3];
	const double n2 = x * x + y * y + z * z + w * w;
	if (n2 > 0.0) { const double inv = 1.0 / sqrt(n2); x *= inv; y *= inv; z *= inv; w *= inv; } // (normalized() leaves a zero quaternion as it is)
	const double tx = 2 * x, ty = 2 * y, tz = 2 * z, twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
	const double m[3][3] = {{1 - (tyy + tzz), txy - twz, txz + twy}, {txy + twz, 1 - (txx + tzz), tyz - twx}, {txz - twy, tyz + twx, 1 - (txx + tyy)}};
	for (int c = 0; c < 3; ++c) for (int i = 0; i < 3; ++i) out[c * 3 + i] = (float)m[i][c];
	for (int i = 0; i < 3; ++i) out[9 + i] = key->T[i];
	return NRS_OK;
}

// CameraKeyframe(matrix, slice, scale, fov, dof), camera_path.h:53: T = m.col(3), R = Quaternionf(m.block<3, 3>(0, 0)).coeffs() (Eigen's conversion: by the trace, else by
// the largest diagonal entry)
int nrs_camera_keyframe_from_matrix(const float matrix[12], float slice, float scale, float fov, float dof, nrs_camera_keyframe* out) {
	if (!matrix || !out) return cam_fail(NRS_ERR_INVALID_ARG, "nrs_camera_keyframe_from_matrix: NULL argument");
	double m[3][3];
	for (int c = 0; c < 3; ++c) for (int i = 0; i < 3; ++i) m[i][c] = (double)matrix[c * 3 + i];
	double q[4]; // x, y, z, w
	double t = m[0][0] + m[1][1] + m[2][2];
	if (t > 0.0) {
		t = sqrt(t + 1.0);
		q[3] = 0.5 * t;
		t = 0.5 / t;
		q[0] = (m[2][1] - m[1][2]) * t; q[1] = (m[0][2] - m[2][0]) * t; q[2] = (m[1][0] - m[0][1]) * t;
	} else {
		int i = 0;
		if (m[1][1] > m[0][0]) i = 1;
		if (m[2][2] > m[i][i]) i = 2;
		const int j = (i + 1) % 3, k = (j + 1) % 3;
		t = sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0);
		q[i] = 0.5 * t;
		t = 0.5 / t;
		q[3] = (m[k][j] - m[j][k]) * t;
		q[j] = (m[j][i] + m[i][j]) * t;
		q[k] = (m[k][i] + m[i][k]) * t;
	}
	for (int i = 0; i < 4; ++i) out->R[i] = (float)q[i];
	for (int i = 0; i < 3; ++i) out->T[i] = matrix[9 + i];
	out->slice = slice; out->scale = scale; out->fov = fov; out->dof = dof;
	return NRS_OK;
}

// CameraPath::eval_camera_path (camera_path.h:74-81) over spline (src/camera_path.cu:50-68, the cubic B-spline branch)
int nrs_camera_path_eval(const nrs_camera_keyframe* keys, uint32_t n_keys, float t, nrs_camera_keyframe* out) {
	if (!out || (n_keys && !keys)) return cam_fail(NRS_ERR_INVALID_ARG, "nrs_camera_path_eval: NULL argument");
	if (!std::isfinite(t)) return cam_fail(NRS_ERR_INVALID_ARG, "nrs_camera_path_eval: t is not finite");
	if (n_keys == 0u) { memset(out, 0, sizeof(*out)); return NRS_OK; }
	if (n_keys > 0x7fffffffu) return cam_fail(NRS_ERR_INVALID_ARG, "nrs_camera_path_eval: too many keyframes");
	t *= (float)(n_keys - 1u);
	const float fl = floorf(t);
	const long long t1 = fabsf(fl) < 4e9f ? (long long)fl : (fl < 0.f ? -4000000000ll : 4000000000ll);
	auto get = [&](long long i) -> const nrs_camera_keyframe& { return keys[i < 0 ? 0 : (i > (long long)n_keys - 1 ? (long long)n_keys - 1 : i)]; };
	const float s = t - fl;
	const float tt = s * s, ttt = s * s * s;
	const float a = (1 - s) * (1 - s) * (1 - s) * (1.f / 6.f);
	const float b = (3.f * ttt - 6.f * tt + 4.f) * (1.f / 6.f);
	const float c = (-3.f * ttt + 3.f * tt + 3.f * s + 1.f) * (1.f / 6.f);
	const float d = ttt * (1.f / 6.f);
	*out = key_sum(key_sum(key_sum(key_scaled(get(t1 - 1), a), key_scaled(get(t1), b)), key_scaled(get(t1 + 1), c)), key_scaled(get(t1 + 2), d));
	return NRS_OK;
}

// src/python_api.cu:148-158
int nrs_motion_views(const float start[12], const float end[12], float shutter_fraction, uint32_t spp_count, uint32_t first_sample, uint32_t spp_total,
                     const int32_t resolution[2], int fov_axis, const nrs_camera_keyframe* keys, uint32_t n_keys, float start_time, float end_time,
                     const nrs_sample_view* base_view, nrs_sample_view* out_views) {
	if (!start || !end || !out_views) return cam_fail(NRS_ERR_INVALID_ARG, "nrs_motion_views: NULL argument (start, end, out_views)");
	if (spp_total == 0u || (uint64_t)first_sample + spp_count > spp_total) return cam_fail(NRS_ERR_INVALID_ARG, "nrs_motion_views: first_sample + spp_count exceeds spp_total");
	if (!std::isfinite(shutter_fraction)) return cam_fail(NRS_ERR_INVALID_ARG, "nrs_motion_views: shutter_fraction is not finite");
	const bool from_path = n_keys > 0u && start_time >= 0.f;
	if (from_path && (!keys || !resolution || (fov_axis != 0 && fov_axis != 1))) return cam_fail(NRS_ERR_INVALID_ARG, "nrs_motion_views: a camera path needs keys, resolution and fov_axis 0 or 1");
	if (from_path && !std::isfinite(end_time)) return cam_fail(NRS_ERR_INVALID_ARG, "nrs_motion_views: end_time is not finite");
	if (!from_path && !base_view) return cam_fail(NRS_ERR_INVALID_ARG, "nrs_motion_views: base_view is NULL and there is no camera path to take fov / dof / slice from");
	for (uint32_t k = 0; k < spp_count; ++k) {
		const uint32_t i = first_sample + k;
		const float start_alpha = ((float)i) / (float)spp_total * shutter_fraction;
		const float end_alpha = ((float)i + 1.0f) / (float)spp_total * shutter_fraction;
		nrs_sample_view v;
		{ const int st = nrs_log_space_lerp(start, end, start_alpha, v.camera_matrix0); if (st != NRS_OK) return st; }
		{ const int st = nrs_log_space_lerp(start, end, end_alpha, v.camera_matrix1); if (st != NRS_OK) return st; }
		if (from_path) { // set_camera_from_time -> set_camera_from_keyframe (src/testbed.cu:2099-2111): fov -> the relative focal length, times resolution[fov_axis] (:2556)
			nrs_camera_keyframe key;
			{ const int st = nrs_camera_path_eval(keys, n_keys, start_time + (end_time - start_time) * (start_alpha + end_alpha) / 2.0f, &key); if (st != NRS_OK) return st; }
			const double rel = 0.5 / tan(0.5 * (double)key.fov * 3.14159265358979323846 / 180.0);
			v.focal_length[0] = v.focal_length[1] = (float)(rel * (double)resolution[fov_axis]);
			v.dof = key.dof;
			v.slice_plane_z = key.slice + key.scale;
		} else {
			v.focal_length[0] = base_view->focal_length[0]; v.focal_length[1] = base_view->focal_length[1];
			v.dof = base_view->dof;
			v.slice_plane_z = base_view->slice_plane_z;
		}
		out_views[k] = v;
	}
	return NRS_OK;
}

} // extern "C"
