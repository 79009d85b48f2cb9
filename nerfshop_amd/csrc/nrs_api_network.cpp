// nrs_api_network.cpp -- the network operators: inference, density, gradients, grid evaluation, selection rays, the Poisson boundary fit, hash-grid encoding, sample traces.
#include "nrs_host.h"
#include "nrs_network.h"
#include "nrs_network_backward.h"

#include <cmath>

using namespace nrs;

extern "C" {

// ---- NerfNetwork operator ------------------------------------------------------------------------------------
static int check_net(nrs_model* m, const void* in, const void* out, const char* who) {
	if (!m || !in || !out) return fail(NRS_ERR_INVALID_ARG, std::string(who) + ": NULL argument");
	if (!m->have_params) return fail(NRS_ERR_STATE, std::string(who) + ": parameters not set (nrs_model_set_params)");
	return NRS_OK;
}
int nrs_network_inference(nrs_model* m, void* stream, uint32_t n, const float* d_in, void* d_out, uint32_t ld_out, int layout) {
	NRS_TRY(check_net(m, d_in, d_out, "nrs_network_inference"));
	if (layout == NRS_PLANES && ld_out < n) return fail(NRS_ERR_INVALID_ARG, "nrs_network_inference: ld_out < n");
	HIP_TRY(hipSetDevice(m->ctx->device));
	NRS_LAUNCH(launch_network(m->dm, kNetInference, n, d_in, NRS_NETWORK_INPUT_FLOATS, d_out, ld_out, layout, m->ctx->n_cus, stream));
	return NRS_OK;
}
int nrs_network_inference_strided(nrs_model* m, void* stream, uint32_t n, const float* d_in, uint32_t ld_in, void* d_out, uint32_t ld_out, int layout) {
	NRS_TRY(check_net(m, d_in, d_out, "nrs_network_inference_strided"));
	if (ld_in < NRS_NETWORK_INPUT_FLOATS) return fail(NRS_ERR_INVALID_ARG, "nrs_network_inference_strided: ld_in < 7");
	if (layout == NRS_PLANES && ld_out < n) return fail(NRS_ERR_INVALID_ARG, "nrs_network_inference_strided: ld_out < n");
	HIP_TRY(hipSetDevice(m->ctx->device));
	NRS_LAUNCH(launch_network(m->dm, kNetInference, n, d_in, ld_in, d_out, ld_out, layout, m->ctx->n_cus, stream, m->n_extra_dims != 0u && ld_in >= 10u));
	return NRS_OK;
}
int nrs_network_density(nrs_model* m, void* stream, uint32_t n, const float* d_in, uint32_t ld_in, void* d_out, uint32_t ld_out, int layout) {
	NRS_TRY(check_net(m, d_in, d_out, "nrs_network_density"));
	if (ld_in < 3) return fail(NRS_ERR_INVALID_ARG, "nrs_network_density: ld_in < 3");
	if (layout == NRS_PLANES && ld_out < n) return fail(NRS_ERR_INVALID_ARG, "nrs_network_density: ld_out < n");
	HIP_TRY(hipSetDevice(m->ctx->device));
	NRS_LAUNCH(launch_network(m->dm, kNetDensity, n, d_in, ld_in, d_out, ld_out, layout, m->ctx->n_cus, stream));
	return NRS_OK;
}
int nrs_network_input_gradient(nrs_model* m, void* stream, uint32_t n, const float* d_in, uint32_t ld_in, float* d_grad_out) {
	NRS_TRY(check_net(m, d_in, d_grad_out, "nrs_network_input_gradient"));
	if (ld_in < 3) return fail(NRS_ERR_INVALID_ARG, "nrs_network_input_gradient: ld_in < 3");
	HIP_TRY(hipSetDevice(m->ctx->device));
	NRS_LAUNCH(launch_network(m->dm, kNetInputGradient, n, d_in, ld_in, d_grad_out, 0, 0, m->ctx->n_cus, stream));
	return NRS_OK;
}
// NerfNetwork::backward (nerf_network_full.h:142-221).  Everything that can be refused is refused before the first HIP call; nothing is allocated and nothing waits.
int nrs_network_backward(nrs_model* m, void* stream, uint32_t n, const float* d_in, uint32_t ld_in, const void* d_dL_doutput_fp16, uint32_t ld_dout, int layout,
                         float* d_dL_dparams, size_t n_params, int accumulate, float* d_dL_dinput) {
	if (!m || !d_dL_dparams || (n && (!d_in || !d_dL_doutput_fp16))) return fail(NRS_ERR_INVALID_ARG, "nrs_network_backward: NULL argument");
	if (ld_in < NRS_NETWORK_INPUT_FLOATS) return fail(NRS_ERR_INVALID_ARG, "nrs_network_backward: ld_in < 7");
	if (layout != NRS_PLANES && layout != NRS_INTERLEAVED) return fail(NRS_ERR_INVALID_ARG, "nrs_network_backward: layout is neither NRS_PLANES nor NRS_INTERLEAVED");
	if (layout == NRS_PLANES && ld_dout < n) return fail(NRS_ERR_INVALID_ARG, "nrs_network_backward: ld_dout < n");
	const size_t expect = (size_t)n_mlp_weights(m->desc, m->n_extra_dims) + (size_t)m->total_entries * 2;
	if (n_params != expect) {
		char buf[160];
		snprintf(buf, sizeof(buf), "nrs_network_backward: n_params is %zu, the description implies %zu", n_params, expect);
		return fail(NRS_ERR_INVALID_ARG, buf);
	}
	const char* field = nullptr;
	if (m->desc.density_hidden_layers != 1u) field = "density_hidden_layers (1 is supported)";
	else if (m->desc.sh_degree != 4u) field = "sh_degree (4 is supported: no backward pass for NerfNetworkNoDir)";
	else if (m->desc.rgb_hidden_layers != 2u) field = "rgb_hidden_layers (2 is supported)";
	else if (m->n_extra_dims != 0u) field = "n_extra_dims (0 is supported: no backward pass with light directions)";
	else if (m->dm.numerics != 0u) field = "nrs_model_set_numerics (NRS_GRID_ACC_FP32 / NRS_MLP_ACC_FP32 are supported)";
	if (field) return fail(NRS_ERR_UNSUPPORTED, std::string("nrs_network_backward: ") + field);
	if (!m->have_params) return fail(NRS_ERR_STATE, "nrs_network_backward: parameters not set (nrs_model_set_params)");
	HIP_TRY(hipSetDevice(m->ctx->device));
	if (!accumulate) HIP_TRY(hipMemsetAsync(d_dL_dparams, 0, n_params * sizeof(float), (hipStream_t)stream)); // EGradientMode::Overwrite
	NRS_LAUNCH(launch_network_backward(m->dm, n, d_in, ld_in, d_dL_doutput_fp16, ld_dout, layout, d_dL_dparams, d_dL_dinput, m->ctx->n_cus, stream));
	return NRS_OK;
}
int nrs_network_visualize_activation(nrs_model* m, void* stream, uint32_t layer, uint32_t dimension, uint32_t n, const float* d_in, float* d_out) {
	NRS_TRY(check_net(m, d_in, d_out, "nrs_network_visualize_activation"));
	if (dimension >= network_layer_width(m->desc, layer, m->n_extra_dims))
		return fail(NRS_ERR_INVALID_ARG, "nrs_network_visualize_activation: no such unit (layers: hash grid 32 | density hidden 64 | rgb input 32, 48 with light directions | one of 64 per rgb hidden layer)");
	HIP_TRY(hipSetDevice(m->ctx->device));
	NRS_LAUNCH(launch_network(m->dm, kNetVisualizeActivation, n, d_in, NRS_NETWORK_INPUT_FLOATS, d_out, 0, 0, m->ctx->n_cus, stream, false, kernel_layer(m->desc, layer), dimension));
	return NRS_OK;
}
int nrs_density_on_grid(nrs_model* m, void* stream, const uint32_t res3d[3], const float aabb_min[3], const float aabb_max[3], int mask_with_density_grid,
                        float* d_out) {
	if (!m || !res3d || !aabb_min || !aabb_max || !d_out) return fail(NRS_ERR_INVALID_ARG, "nrs_density_on_grid: NULL argument");
	if (!m->have_params) return fail(NRS_ERR_STATE, "nrs_density_on_grid: parameters not set (nrs_model_set_params)");
	if ((uint64_t)res3d[0] * res3d[1] * res3d[2] > 0x7fffffffull) return fail(NRS_ERR_INVALID_ARG, "nrs_density_on_grid: more than 2^31 grid points");
	HIP_TRY(hipSetDevice(m->ctx->device));
	NRS_LAUNCH(launch_grid_eval(m->dm, kGridDensity, res3d, aabb_min, aabb_max, nullptr, mask_with_density_grid ? m->d_density_grid.get() : nullptr, d_out, m->ctx->n_cus, stream));
	return NRS_OK;
}
int nrs_rgba_on_grid(nrs_model* m, void* stream, const uint32_t res3d[3], const float render_aabb_min[3], const float render_aabb_max[3],
                     const float ray_dir[3], float* d_out_rgba) {
	if (!m || !res3d || !render_aabb_min || !render_aabb_max || !ray_dir || !d_out_rgba) return fail(NRS_ERR_INVALID_ARG, "nrs_rgba_on_grid: NULL argument");
	if (!m->have_params) return fail(NRS_ERR_STATE, "nrs_rgba_on_grid: parameters not set (nrs_model_set_params)");
	if ((uint64_t)res3d[0] * res3d[1] * res3d[2] > 0x7fffffffull) return fail(NRS_ERR_INVALID_ARG, "nrs_rgba_on_grid: more than 2^31 grid points");
	HIP_TRY(hipSetDevice(m->ctx->device));
	const float dir01[3] = {(ray_dir[0] + 1.0f) * 0.5f, (ray_dir[1] + 1.0f) * 0.5f, (ray_dir[2] + 1.0f) * 0.5f}; // warp_direction, not normalised (tn:430)
	NRS_LAUNCH(launch_grid_eval(m->dm, kGridRgba, res3d, render_aabb_min, render_aabb_max, dir01, nullptr, d_out_rgba, m->ctx->n_cus, stream));
	return NRS_OK;
}
int nrs_project_selection_pixels(nrs_model* m, void* stream, const nrs_render_params* p, const int32_t* d_pixels_xy, uint32_t n_pixels,
                                 float transmittance_threshold, float* d_positions, uint32_t* d_cells, uint8_t* d_found) {
	if (!m || !p || (n_pixels && (!d_pixels_xy || !d_positions || !d_cells || !d_found)))
		return fail(NRS_ERR_INVALID_ARG, "nrs_project_selection_pixels: NULL argument");
	if (!m->have_params) return fail(NRS_ERR_STATE, "nrs_project_selection_pixels: parameters not set (nrs_model_set_params)");
	if (!m->have_bitfield) return fail(NRS_ERR_STATE, "nrs_project_selection_pixels: occupancy not set (nrs_model_set_density_bitfield/_grid)");
	NRS_TRY(check_march_params(*p, "nrs_project_selection_pixels"));
	HIP_TRY(hipSetDevice(m->ctx->device));
	NRS_LAUNCH(launch_selection_rays(m->dm, *p, d_pixels_xy, n_pixels, transmittance_threshold, d_positions, d_cells, d_found, stream));
	return NRS_OK;
}
// Sampling directions of compute_poisson_boundary (growing_selection.cu:2241-2261), on the host with the host's libm as the
// reference does; jitter = the two (float)std::rand() / RAND_MAX draws per sample, supplied by the caller.
void nrs_poisson_sample_coords(const float* vertices, uint32_t n_verts, uint32_t sh_width, uint32_t hemisphere_width, const float* jitter,
                               const float aabb_min[3], const float aabb_max[3], float* coords7) {
	const uint32_t n_sh = sh_width * sh_width;
	for (uint32_t k = 0; k < n_verts; ++k)
		for (uint32_t i = 0; i < sh_width; ++i)
			for (uint32_t j = 0; j < sh_width; ++j) {
				const size_t s = (size_t)n_sh * k + (size_t)i * sh_width + j;
				const float u = ((float)i + jitter[2 * s]) / (float)(int)hemisphere_width;
				const float v = ((float)j + jitter[2 * s + 1]) / (float)(int)hemisphere_width;
				const float theta = (float)(2.f * M_PI * v);
				const float phi = acosf(2.f * u - 1.f);
				const float x = cosf(theta) * sinf(phi), y = sinf(theta) * sinf(phi), z = cosf(phi);
				float* c = coords7 + s * 7;
				for (int a = 0; a < 3; ++a) c[a] = (vertices[3 * k + a] - aabb_min[a]) / (aabb_max[a] - aabb_min[a]); // warp_position
				c[3] = 0.f;
				c[4] = (x + 1.f) * 0.5f; c[5] = (y + 1.f) * 0.5f; c[6] = (z + 1.f) * 0.5f; // warp_direction
			}
}
int nrs_poisson_boundary(nrs_model* m, const float* h_vertices, uint32_t n_verts, uint32_t sh_width, uint32_t hemisphere_width, const float* h_jitter,
                         int is_inside, float* h_density_out, float* h_sh_out) {
	if (!m || (n_verts && (!h_vertices || !h_jitter || !h_density_out || !h_sh_out))) return fail(NRS_ERR_INVALID_ARG, "nrs_poisson_boundary: NULL argument");
	if (!m->have_params) return fail(NRS_ERR_STATE, "nrs_poisson_boundary: parameters not set (nrs_model_set_params)");
	if (is_inside && !m->have_bitfield) return fail(NRS_ERR_STATE, "nrs_poisson_boundary: occupancy not set (nrs_model_set_density_bitfield/_grid)");
	if (sh_width == 0 || sh_width > 64 || hemisphere_width == 0) return fail(NRS_ERR_INVALID_ARG, "nrs_poisson_boundary: sampling widths out of range (1..64)");
	if (n_verts == 0) return NRS_OK;
	HIP_TRY(hipSetDevice(m->ctx->device));
	const uint32_t n_sh = sh_width * sh_width;
	const size_t n = (size_t)n_verts * n_sh;
	if (n > 0x7fffffffull) return fail(NRS_ERR_INVALID_ARG, "nrs_poisson_boundary: too many samples");
	std::vector<float> coords(n * 7);
	nrs_poisson_sample_coords(h_vertices, n_verts, sh_width, hemisphere_width, h_jitter, m->dm.aabb.mn, m->dm.aabb.mx, coords.data());
	DeviceBuffer<float> d_coords, d_density, d_sh;
	DeviceBuffer<uint16_t> d_net; // fp16, 16 channels per sample
	hipError_t he = d_coords.alloc(n * 7);
	if (he == hipSuccess) he = d_net.alloc(n * 16);
	if (he == hipSuccess) he = d_density.alloc(n_verts);
	if (he == hipSuccess) he = d_sh.alloc((size_t)n_verts * 27);
	if (he != hipSuccess) return fail_hip(he, "nrs_poisson_boundary: device allocation");
	if (hipMemcpy(d_coords.get(), coords.data(), n * 7 * 4, hipMemcpyHostToDevice) != hipSuccess) return fail(NRS_ERR_HIP, "nrs_poisson_boundary: upload");
	NRS_LAUNCH(launch_network(m->dm, kNetInference, (uint32_t)n, d_coords.get(), NRS_NETWORK_INPUT_FLOATS, d_net.get(), 16, NRS_INTERLEAVED, m->ctx->n_cus, nullptr));
	NRS_LAUNCH(launch_poisson_fit(m->dm, n_verts, n_sh, d_coords.get(), d_net.get(), is_inside, (float)(4 * M_PI / n_sh), d_density.get(), d_sh.get(), nullptr));
	if (hipMemcpy(h_density_out, d_density.get(), (size_t)n_verts * 4, hipMemcpyDeviceToHost) != hipSuccess ||
	    hipMemcpy(h_sh_out, d_sh.get(), (size_t)n_verts * 27 * 4, hipMemcpyDeviceToHost) != hipSuccess)
		return fail(NRS_ERR_HIP, "nrs_poisson_boundary: download");
	return NRS_OK;
}
int nrs_hashgrid_encode(nrs_model* m, void* stream, uint32_t n, const float* d_in, uint32_t ld_in, void* d_out) {
	NRS_TRY(check_net(m, d_in, d_out, "nrs_hashgrid_encode"));
	if (ld_in < 3) return fail(NRS_ERR_INVALID_ARG, "nrs_hashgrid_encode: ld_in < 3");
	HIP_TRY(hipSetDevice(m->ctx->device));
	NRS_LAUNCH(launch_network(m->dm, kNetEncode, n, d_in, ld_in, d_out, 0, NRS_INTERLEAVED, m->ctx->n_cus, stream));
	return NRS_OK;
}

int nrs_trace_samples(nrs_model* m, const nrs_render_params* p, void* stream, uint32_t n_pixels, const uint32_t* d_pixel_idx, uint32_t max_samples,
                      float* d_t, float* d_dt, uint32_t* d_count) {
	if (!m || !p || !d_pixel_idx || !d_t || !d_dt || !d_count) return fail(NRS_ERR_INVALID_ARG, "nrs_trace_samples: NULL argument");
	if (!m->have_bitfield) return fail(NRS_ERR_STATE, "nrs_trace_samples: occupancy not set");
	NRS_TRY(check_march_params(*p, "nrs_trace_samples"));
	HIP_TRY(hipSetDevice(m->ctx->device));
	NRS_LAUNCH(launch_trace_samples(model_for_launch(m, *p), *p, n_pixels, d_pixel_idx, max_samples, d_t, d_dt, d_count, stream));
	return NRS_OK;
}

} // extern "C"
