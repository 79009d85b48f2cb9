// nrs_compat.hpp -- header-only C++ adaptor over the C-ABI of nrs.h that gives the render path the SHAPE of the reference's
// own C++ interfaces, so call sites in src/testbed.cu / src/testbed_nerf.cu map 1:1:
//
//   ngp::NerfNetwork<T>        include/neural-graphics-primitives/nerf_network.h:86        -> nrs::compat::NerfNetwork
//   ngp::CageDeformation       include/neural-graphics-primitives/editing/edit_operator.h  -> nrs::compat::CageDeformation
//   ngp::CudaRenderBuffer      include/neural-graphics-primitives/render_buffer.h:164      -> nrs::compat::RenderBuffer (view)
//   ngp::Testbed::render_nerf  src/testbed_nerf.cu:3066                                    -> nrs::compat::Testbed::render_nerf
//   ngp::Testbed::render_to_cpu src/python_api.cu:129-175                                  -> nrs::compat::Testbed::render_to_cpu (+ load_camera_path,
//                                                                                             set_camera_from_time, apply_camera_smoothing)
//   ngp::Testbed::marching_cubes src/testbed_nerf.cu:4614 (+ compute_and_save_marching_cubes_mesh, get_marching_cubes_res) -> nrs::compat::Testbed::marching_cubes
//   ngp::GrowingSelection (RegionGrowing, CorrectMMOperations) src/editing/tools/growing_selection.cu:2083-2162, region_growing.cu -> nrs::compat::GrowingSelection
//
// No Eigen / tiny-cuda-nn types: matrices are column-major float arrays (what Eigen::Matrix<float,3,4>::data() yields),
// streams are passed as void* (hipStream_t), errors become std::runtime_error (the reference throws from CUDA_CHECK_THROW).
#pragma once
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "nrs.h"

namespace nrs {
namespace compat {

inline void check(int status, const char* what) {
	if (status != NRS_OK) throw std::runtime_error(std::string(what) + ": " + nrs_last_error());
}

class Context {
public:
	explicit Context(int device = 0) { check(nrs_ctx_create(device, &m_ctx), "nrs_ctx_create"); }
	~Context() { nrs_ctx_destroy(m_ctx); }
	Context(const Context&) = delete;
	Context& operator=(const Context&) = delete;
	nrs_ctx* get() const { return m_ctx; }

private:
	nrs_ctx* m_ctx = nullptr;
};

// Non-owning matrix views with tcnn's meaning: GPUMatrixDynamic<float> (column-major, m rows = floats per sample) and
// GPUMatrixDynamic<T> with a selectable layout for the fp16 output.
struct InputMatrix {
	const float* data;  // device
	uint32_t rows;      // floats per sample (7 for inference, 3..7 for density)
	uint32_t n;         // samples (columns)
};
struct OutputMatrix {
	void* data;         // device, fp16
	uint32_t rows;      // 16
	uint32_t n;         // columns allocated (n_el >= samples for the planes layout)
	nrs_layout layout;  // NRS_PLANES = tcnn RM (row-major 16 x n), NRS_INTERLEAVED = tcnn CM
};

class NerfNetwork {
public:
	// n_extra_dims: 0, or 3 for a network trained with light directions (dataset.has_light_dirs, testbed.cu:2318)
	NerfNetwork(Context& ctx, const nrs_model_desc& desc, uint32_t n_extra_dims = 0) : m_desc(desc) {
		check(nrs_model_create_ex(ctx.get(), &desc, n_extra_dims, &m_model), "nrs_model_create_ex");
	}
	~NerfNetwork() { nrs_model_destroy(m_model); }
	NerfNetwork(const NerfNetwork&) = delete;
	NerfNetwork& operator=(const NerfNetwork&) = delete;

	// tcnn::Network interface subset used on the path (nerf_network.h:97-120)
	uint32_t padded_output_width() const { return NRS_NETWORK_OUTPUT_WIDTH; }
	uint32_t input_width() const { return NRS_NETWORK_INPUT_FLOATS; }
	uint32_t n_extra_dims() const { return (uint32_t)nrs_model_n_extra_dims(m_model); }
	size_t n_params() const { return nrs_model_n_params_ex(&m_desc, n_extra_dims()); }

	// set_params(params, inference_params, ...) of the reference takes device pointers into the trainer's blob; here the fp16
	// blob (density MLP | rgb MLP | hash grid, nerf_network_full.h:316-349) is handed over from the host once.
	void set_params(const void* h_params_fp16, size_t n) { check(nrs_model_set_params(m_model, h_params_fp16, n), "nrs_model_set_params"); }
	// ... or, as in the reference, from device pointers (call again after every optimiser step: nrs.h)
	void set_params_device(const void* d_params_fp16, size_t n, void* stream) { check(nrs_model_set_params_device(m_model, d_params_fp16, n, stream), "nrs_model_set_params_device"); }
	// budget of the cell-record cache (no counterpart in the reference; results do not depend on it), 0 = off
	void set_cell_cache(size_t max_bytes) { check(nrs_model_set_cell_cache(m_model, max_bytes), "nrs_model_set_cell_cache"); }

	void inference_mixed_precision(void* stream, const InputMatrix& input, OutputMatrix& output, bool /*use_inference_params*/ = true) {
		if (input.rows != NRS_NETWORK_INPUT_FLOATS) throw std::runtime_error("NerfNetwork::inference_mixed_precision: input must have 7 rows");
		check(nrs_network_inference(m_model, stream, input.n, input.data, output.data, output.n, output.layout), "nrs_network_inference");
	}
	void density(void* stream, const InputMatrix& input, OutputMatrix& output, bool /*use_inference_params*/ = true) {
		check(nrs_network_density(m_model, stream, input.n, input.data, input.rows, output.data, output.n, output.layout), "nrs_network_density");
	}
	// tcnn::DifferentiableObject::input_gradient(stream, dim, input, d_dinput) as the path calls it (dim = 3: the density; testbed_nerf.cu:2924, :4491).
	// d_grad: [n x 3] f32, the position rows of the reference's gradient matrix (the dt / direction rows are zero there).
	void input_gradient(void* stream, uint32_t dim, const InputMatrix& input, float* d_grad_nx3) {
		if (dim != 3) throw std::runtime_error("NerfNetwork::input_gradient: the render path differentiates output 3 (the density) only");
		check(nrs_network_input_gradient(m_model, stream, input.n, input.data, input.rows, d_grad_nx3), "nrs_network_input_gradient");
	}
	// tcnn::DifferentiableObject::backward(stream, ctx, input, output, dL_doutput, dL_dinput, use_inference_params, param_gradients_mode) (nerf_network_full.h:142-221).
	// The forward context and `output` of the reference carry the activations; here the kernel recomputes them, so both are absent.  d_dL_dparams: n_params() floats,
	// fp32, the blob's order; d_dL_dinput: null, or [n x input.rows] f32 (position rows only: nrs.h).  accumulate = EGradientMode::Accumulate, else Overwrite.
	void backward(void* stream, const InputMatrix& input, const OutputMatrix& dL_doutput, float* d_dL_dparams, float* d_dL_dinput = nullptr, bool accumulate = false) {
		check(nrs_network_backward(m_model, stream, input.n, input.data, input.rows, dL_doutput.data, dL_doutput.n, dL_doutput.layout, d_dL_dparams, n_params(),
		                           accumulate ? 1 : 0, d_dL_dinput), "nrs_network_backward");
	}
	// generate_training_samples_nerf from the ray on (testbed_nerf.cu:1188-1246; nrs.h "training rays"): coords_out [max_samples x rows] f32, rows >= 7
	void training_samples(void* stream, uint32_t n_rays, const float* d_rays, const float* d_jitter, float cone_angle_constant, uint32_t max_samples,
	                      float* d_coords_out, uint32_t rows, uint32_t* d_numsteps_out, uint32_t* d_ray_indices_out, uint32_t* d_counters) {
		check(nrs_training_samples(m_model, stream, n_rays, d_rays, d_jitter, cone_angle_constant, max_samples, d_coords_out, rows, d_numsteps_out, d_ray_indices_out,
		                           d_counters), "nrs_training_samples");
	}
	// compute_loss_kernel_train_nerf (testbed_nerf.cu:1685-1985): coords = the samples' records (coords.n of them), output what inference wrote for them,
	// dL_doutput and d_coords_out the compacted results (params.max_samples_compacted records)
	void ray_loss(void* stream, const nrs_ray_loss_params& params, uint32_t n_rays, const uint32_t* d_ray_counter, const uint32_t* d_numsteps, const InputMatrix& coords,
	              const OutputMatrix& output, const float* d_target_rgba, const float* d_background, const float* d_ray_origins, uint32_t* d_numsteps_out,
	              float* d_coords_out, OutputMatrix& dL_doutput, float* d_loss, uint32_t* d_counter_out) {
		check(nrs_ray_loss(m_model, stream, &params, n_rays, d_ray_counter, d_numsteps, coords.n, coords.data, coords.rows, output.data, output.n, output.layout,
		                   d_target_rgba, d_background, d_ray_origins, d_numsteps_out, d_coords_out, dL_doutput.data, dL_doutput.n, dL_doutput.layout, d_loss,
		                   d_counter_out), "nrs_ray_loss");
	}
	// ray_loss with the two additions of the trainable environment map (nrs_ray_loss_ex): the linear background a ray sees (Envmap::background) and the per-slot record
	// the envmap's gradient reads (NRS_RAY_AUX_WORDS words per slot); either may be NULL
	void ray_loss_ex(void* stream, const nrs_ray_loss_params& params, uint32_t n_rays, const uint32_t* d_ray_counter, const uint32_t* d_numsteps, const InputMatrix& coords,
	                 const OutputMatrix& output, const float* d_target_rgba, const float* d_background, const float* d_ray_origins, uint32_t* d_numsteps_out,
	                 float* d_coords_out, OutputMatrix& dL_doutput, float* d_loss, uint32_t* d_counter_out, const float* d_background_linear, uint32_t* d_ray_aux) {
		check(nrs_ray_loss_ex(m_model, stream, &params, n_rays, d_ray_counter, d_numsteps, coords.n, coords.data, coords.rows, output.data, output.n, output.layout,
		                      d_target_rgba, d_background, d_ray_origins, d_numsteps_out, d_coords_out, dL_doutput.data, dL_doutput.n, dL_doutput.layout, d_loss,
		                      d_counter_out, d_background_linear, d_ray_aux), "nrs_ray_loss_ex");
	}
	// tcnn::Network::visualize_activation(stream, layer, dimension, input, output): the activation itself, f32 [n] (testbed_nerf.cu:2926, :3159)
	void visualize_activation(void* stream, uint32_t layer, uint32_t dimension, const InputMatrix& input, float* d_out_n) {
		if (input.rows != NRS_NETWORK_INPUT_FLOATS) throw std::runtime_error("NerfNetwork::visualize_activation: input must have 7 rows");
		check(nrs_network_visualize_activation(m_model, stream, layer, dimension, input.n, input.data, d_out_n), "nrs_network_visualize_activation");
	}

	// Testbed::m_nerf.density_grid_bitfield / update_density_grid_mean_and_bitfield
	void set_density_bitfield(const uint8_t* h_bits, size_t n) { check(nrs_model_set_density_bitfield(m_model, h_bits, n), "nrs_model_set_density_bitfield"); }
	void set_density_grid(const float* h_grid, size_t n) { check(nrs_model_set_density_grid(m_model, h_grid, n), "nrs_model_set_density_grid"); }

	void get_density_grid(float* h_grid, size_t n) { check(nrs_model_get_density_grid(m_model, h_grid, n), "nrs_model_get_density_grid"); }

	nrs_model* get() const { return m_model; }
	const nrs_model_desc& desc() const { return m_desc; }

private:
	nrs_model_desc m_desc;
	nrs_model* m_model = nullptr;
};

// tcnn::Trainer's optimiser half as the training loop uses it: m_trainer->optimizer_step(stream, LOSS_SCALE) (testbed_nerf.cu:3761) over the optimiser of
// configs/nerf/base.json (nrs.h "optimiser").  Bound to a network, a step writes the parameters the network reads: no set_params call follows it.  The gradient buffer is
// the caller's (n_params() floats, what NerfNetwork::backward accumulates into); the learning rate is the caller's schedule (exponential_decay_lr).
class Optimizer {
public:
	static nrs_adam_params base_params() { return nrs_adam_params{(uint32_t)sizeof(nrs_adam_params), 0.9f, 0.99f, 1e-15f, 1e-6f, 1.0f, 0.95f}; }
	Optimizer(NerfNetwork& network, const nrs_adam_params& params) { check(nrs_optimizer_create_for_model(network.get(), &params, &m_opt), "nrs_optimizer_create_for_model"); }
	Optimizer(Context& ctx, size_t n_params, size_t n_matrix, const nrs_adam_params& params) {
		check(nrs_optimizer_create(ctx.get(), n_params, n_matrix, &params, &m_opt), "nrs_optimizer_create");
	}
	~Optimizer() { nrs_optimizer_destroy(m_opt); }
	Optimizer(const Optimizer&) = delete;
	Optimizer& operator=(const Optimizer&) = delete;

	size_t n_params() const { return nrs_optimizer_n_params(m_opt, nullptr); }
	// Trainer::set_params_full_precision / initialize_params: fp32 master weights from the host or the device
	void set_weights(const float* weights, bool on_device, void* stream) { check(nrs_optimizer_set_weights(m_opt, weights, on_device ? 1 : 0, stream), "nrs_optimizer_set_weights"); }
	void set_gradients(float* d_grad, bool zero_after_step = true) { m_grad = d_grad; m_zero_grad = zero_after_step; }
	void set_learning_rate(float lr) { m_lr = lr; }
	float learning_rate() const { return m_lr; }
	// ExponentialDecay(decay_start, decay_interval, decay_base) over `base`, for the step after steps_done finished ones
	static float exponential_decay_lr(float base, uint32_t decay_start, uint32_t decay_interval, float decay_base, uint32_t steps_done) {
		return nrs_exponential_decay_lr(base, decay_start, decay_interval, decay_base, steps_done);
	}
	void step(void* stream, float loss_scale) {
		if (!m_grad) throw std::runtime_error("Optimizer::step: no gradient buffer (set_gradients)");
		check(nrs_optimizer_step(m_opt, stream, m_grad, loss_scale, m_lr, m_zero_grad ? 1 : 0), "nrs_optimizer_step");
	}
	uint32_t step() const { return nrs_optimizer_step_count(m_opt); }
	// the blob as fp16 on the device: the weights, or the EMA a second network renders with (NerfNetwork::set_params_device)
	void export_fp16(nrs_optimizer_export which, void* d_out_fp16, void* stream) { check(nrs_optimizer_export_fp16(m_opt, which, d_out_fp16, stream), "nrs_optimizer_export_fp16"); }
	void get_state(nrs_optimizer_state which, void* h_out, size_t n) { check(nrs_optimizer_get_state(m_opt, which, h_out, n), "nrs_optimizer_get_state"); }
	void set_state(nrs_optimizer_state which, const void* h_in, size_t n) { check(nrs_optimizer_set_state(m_opt, which, h_in, n), "nrs_optimizer_set_state"); }
	nrs_optimizer* get() const { return m_opt; }

private:
	nrs_optimizer* m_opt = nullptr;
	float* m_grad = nullptr;
	float m_lr = 1e-2f;
	bool m_zero_grad = true;
};

// nrs_image_metrics_params with run.py's defaults: a black, opaque background unless background_rgba is given
inline nrs_image_metrics_params image_metrics_params(nrs_color_space color_space, const float* background_rgba, nrs_image_format reference_format) {
	nrs_image_metrics_params p{(uint32_t)sizeof(nrs_image_metrics_params), (uint32_t)color_space, {0.0f, 0.0f, 0.0f, 1.0f}, (uint32_t)reference_format};
	if (background_rgba) std::memcpy(p.background_color, background_rgba, sizeof(p.background_color));
	return p;
}

// NerfDataset on the device (nerf_loader.h: images_data, xforms, metadata) with the front half of generate_training_samples_nerf.  A thin owner of the handle: images arrive
// decoded (the loader and its file formats stay with the caller).
class Dataset {
public:
	Dataset(Context& ctx, uint32_t n_images, uint32_t width, uint32_t height) { check(nrs_dataset_create(ctx.get(), n_images, width, height, &m_ds), "nrs_dataset_create"); }
	~Dataset() { nrs_dataset_destroy(m_ds); }
	Dataset(const Dataset&) = delete;
	Dataset& operator=(const Dataset&) = delete;

	static nrs_training_camera camera() { // identity transforms, principal point in the centre, no distortion: fill in the rest
		nrs_training_camera c{};
		c.struct_size = (uint32_t)sizeof(nrs_training_camera);
		c.xform_start[0] = c.xform_start[4] = c.xform_start[8] = c.xform_end[0] = c.xform_end[4] = c.xform_end[8] = 1.f;
		c.principal_point[0] = c.principal_point[1] = 0.5f;
		return c;
	}
	void set_image(uint32_t index, nrs_image_format format, const void* pixels, bool on_device, void* stream, uint32_t flags = 0, uint32_t mask_color = 0) {
		check(nrs_dataset_set_image(m_ds, index, format, pixels, on_device ? 1 : 0, flags, mask_color, stream), "nrs_dataset_set_image");
	}
	void get_image(uint32_t index, void* h_out_fp16) { check(nrs_dataset_get_image(m_ds, index, h_out_fp16), "nrs_dataset_get_image"); }
	void set_camera(uint32_t index, const nrs_training_camera& camera) { check(nrs_dataset_set_camera(m_ds, index, &camera), "nrs_dataset_set_camera"); }
	// the rays of one training step: m_rng's (state, inc), the rays of the steps before; d_background may be NULL without random_bg_color, d_pixels always
	void rays(void* stream, uint32_t n_rays, uint32_t n_rays_total, uint64_t rng_state, uint64_t rng_inc, float* d_rays, float* d_jitter, float* d_target_rgba,
	          float* d_background, uint32_t* d_pixels = nullptr, bool snap_to_pixel_centers = true, bool random_bg_color = true) {
		const nrs_dataset_rays_params p{(uint32_t)sizeof(nrs_dataset_rays_params), n_rays_total, rng_state, rng_inc, snap_to_pixel_centers ? 1u : 0u, random_bg_color ? 1u : 0u};
		check(nrs_dataset_rays(m_ds, stream, &p, n_rays, d_rays, d_jitter, d_target_rgba, d_background, d_pixels), "nrs_dataset_rays");
	}
	void mark_untrained(NerfNetwork& network, bool clear_visible_voxels, void* stream) {
		check(nrs_dataset_mark_untrained(network.get(), m_ds, clear_visible_voxels ? 1 : 0, stream), "nrs_dataset_mark_untrained");
	}
	// the training error map (m_nerf.training.error_map): its cells, the CDFs built from them, and rays drawn in proportion to them -- rays() with two switches and
	// two more outputs, d_xy [n x 2] (what error_map_accumulate reads) and d_pdf [n]
	void error_map_reset(uint32_t res_x, uint32_t res_y, void* stream) { check(nrs_dataset_error_map_reset(m_ds, res_x, res_y, stream), "nrs_dataset_error_map_reset"); }
	void error_map_set(uint32_t res_x, uint32_t res_y, const float* h_data) { check(nrs_dataset_error_map_set(m_ds, res_x, res_y, h_data), "nrs_dataset_error_map_set"); }
	size_t error_map_get(nrs_error_map_what what, void* h_out) { // h_out == nullptr: the number of elements alone
		size_t count = 0;
		check(nrs_dataset_error_map_get(m_ds, what, h_out, &count), "nrs_dataset_error_map_get");
		return count;
	}
	void error_map_accumulate(void* stream, uint32_t n_rays, const uint32_t* d_ray_counter, const uint32_t* d_ray_indices, const float* d_loss, const float* d_xy,
	                          const uint32_t* d_pixels, const float* d_pdf = nullptr, float* d_loss_weighted = nullptr) {
		check(nrs_dataset_error_map_accumulate(m_ds, stream, n_rays, d_ray_counter, d_ray_indices, d_loss, d_xy, d_pixels, d_pdf, d_loss_weighted), "nrs_dataset_error_map_accumulate");
	}
	void error_map_build_cdfs(void* stream) { check(nrs_dataset_error_map_build_cdfs(m_ds, stream), "nrs_dataset_error_map_build_cdfs"); }
	void rays_by_error(void* stream, uint32_t n_rays, uint32_t n_rays_total, uint64_t rng_state, uint64_t rng_inc, bool sample_images, bool sample_pixels, float* d_rays,
	                   float* d_jitter, float* d_target_rgba, float* d_background, uint32_t* d_pixels, float* d_xy, float* d_pdf, bool snap_to_pixel_centers = true,
	                   bool random_bg_color = true) {
		const nrs_dataset_rays_ex_params p{(uint32_t)sizeof(nrs_dataset_rays_ex_params), n_rays_total, rng_state, rng_inc, snap_to_pixel_centers ? 1u : 0u, random_bg_color ? 1u : 0u,
		                                   sample_images ? 1u : 0u, sample_pixels ? 1u : 0u};
		check(nrs_dataset_rays_ex(m_ds, stream, &p, n_rays, d_rays, d_jitter, d_target_rgba, d_background, d_pixels, d_xy, d_pdf), "nrs_dataset_rays_ex");
	}
	// PSNR's squared error and SSIM of d_image (f32x4 per pixel, linear: an accumulate buffer) against image `index`, read where it lies (nrs_dataset_image_metrics):
	// *d_result on the device, the two maps [height x width] when not null; nothing waits for the device
	void image_metrics(uint32_t index, void* stream, const float* d_image, nrs_image_metrics_result* d_result, nrs_color_space color_space = NRS_COLOR_LINEAR,
	                   const float* background_rgba = nullptr, float* d_ssim_map = nullptr, float* d_sq_err_map = nullptr) {
		const nrs_image_metrics_params p = image_metrics_params(color_space, background_rgba, NRS_IMAGE_RGBA16F_LINEAR);
		check(nrs_dataset_image_metrics(m_ds, index, stream, d_image, &p, d_result, d_ssim_map, d_sq_err_map), "nrs_dataset_image_metrics");
	}
	nrs_dataset* get() const { return m_ds; }

private:
	nrs_dataset* m_ds = nullptr;
};

// Testbed::m_envmap as the training loop uses it (testbed.h: envmap, its loss and optimiser; nrs.h "the environment map"): res_x x res_y RGBA texels trained behind the
// last sample of every ray.  A fresh map is all zeros.  The learning rate is the caller's schedule (envmap_lr: base.json's envmap block).
class Envmap {
public:
	static nrs_adam_params base_params() { // base.json's envmap optimiser: Ema(0.99) over Adam(0.9, 0.99, 1e-10)
		nrs_adam_params p{};
		nrs_envmap_default_adam_params(&p);
		return p;
	}
	static nrs_envmap_accumulate_params accumulate_params(const nrs_ray_loss_params& loss, nrs_loss_type envmap_loss_type = NRS_LOSS_RELATIVE_L2) {
		return nrs_envmap_accumulate_params{(uint32_t)sizeof(nrs_envmap_accumulate_params), loss.loss_type, (uint32_t)envmap_loss_type, loss.loss_scale,
		                                    loss.train_in_linear_colors};
	}
	// ExponentialDecay(10000, 5000, 0.33) over 1e-2, for the step after steps_done finished ones
	static float envmap_lr(uint32_t steps_done) { return nrs_exponential_decay_lr(1e-2f, 10000, 5000, 0.33f, steps_done); }

	Envmap(Context& ctx, uint32_t res_x, uint32_t res_y) { check(nrs_envmap_create(ctx.get(), res_x, res_y, nullptr, &m_env), "nrs_envmap_create"); }
	Envmap(Context& ctx, uint32_t res_x, uint32_t res_y, const nrs_adam_params& params) { check(nrs_envmap_create(ctx.get(), res_x, res_y, &params, &m_env), "nrs_envmap_create"); }
	~Envmap() { nrs_envmap_destroy(m_env); }
	Envmap(const Envmap&) = delete;
	Envmap& operator=(const Envmap&) = delete;

	size_t n_floats() const {
		uint32_t x = 0, y = 0;
		check(nrs_envmap_resolution(m_env, &x, &y), "nrs_envmap_resolution");
		return (size_t)4 * x * y;
	}
	void set_texels(const float* texels, bool on_device, void* stream) { check(nrs_envmap_set_texels(m_env, texels, on_device ? 1 : 0, stream), "nrs_envmap_set_texels"); }
	void get(nrs_envmap_what which, void* h_out) { check(nrs_envmap_get(m_env, which, h_out, n_floats()), "nrs_envmap_get"); }
	// the EMA (params_inference) or the live texels (params) into d_out [res_y][res_x][4]: what nrs_render_params::d_envmap takes
	void export_texels(bool ema, float* d_out, void* stream) { check(nrs_envmap_export(m_env, ema ? 1 : 0, d_out, stream), "nrs_envmap_export"); }
	// per ray slot: the linear background behind the ray (for NerfNetwork::ray_loss_ex) and the lookup's footprint (for accumulate)
	void background(void* stream, uint32_t n_rays, const uint32_t* d_ray_counter, const uint32_t* d_ray_indices, const float* d_rays, const float* d_background,
	                const float* default_background, float* d_background_linear, int32_t* d_footprint) {
		check(nrs_envmap_background(m_env, stream, n_rays, d_ray_counter, d_ray_indices, d_rays, d_background, default_background, d_background_linear, d_footprint),
		      "nrs_envmap_background");
	}
	void accumulate(void* stream, const nrs_envmap_accumulate_params& params, uint32_t n_rays, const uint32_t* d_ray_counter, const uint32_t* d_numsteps_out,
	                const uint32_t* d_ray_aux, const float* d_background_linear, const int32_t* d_footprint) {
		check(nrs_envmap_accumulate(m_env, stream, &params, n_rays, d_ray_counter, d_numsteps_out, d_ray_aux, d_background_linear, d_footprint), "nrs_envmap_accumulate");
	}
	void step(void* stream, float loss_scale, float learning_rate) { check(nrs_envmap_step(m_env, stream, loss_scale, learning_rate), "nrs_envmap_step"); }
	uint32_t step() const { return nrs_envmap_step_count(m_env); }
	nrs_envmap* get() const { return m_env; }

private:
	nrs_envmap* m_env = nullptr;
};

// m_nerf.training.cam_exposure with optimize_exposure (testbed.h; nrs.h "per-image exposure"): a log2 exposure per training image and channel, trained through the
// target colour.  Fresh exposures are zero.  The learning rate is the caller's: the reference passes the network optimiser's current one.
class Exposure {
public:
	static nrs_exposure_params default_params() { // the per-image AdamOptimizer (0.9, 0.99, 1e-8), exposure_l2_reg 0, n_steps_between_cam_updates 16
		nrs_exposure_params p{};
		nrs_exposure_default_params(&p);
		return p;
	}
	static nrs_exposure_accumulate_params accumulate_params(const nrs_ray_loss_params& loss) {
		return nrs_exposure_accumulate_params{(uint32_t)sizeof(nrs_exposure_accumulate_params), loss.loss_scale, loss.train_in_linear_colors};
	}

	Exposure(Context& ctx, uint32_t n_images) { check(nrs_exposure_create(ctx.get(), n_images, nullptr, &m_exp), "nrs_exposure_create"); }
	Exposure(Context& ctx, uint32_t n_images, const nrs_exposure_params& params) { check(nrs_exposure_create(ctx.get(), n_images, &params, &m_exp), "nrs_exposure_create"); }
	~Exposure() { nrs_exposure_destroy(m_exp); }
	Exposure(const Exposure&) = delete;
	Exposure& operator=(const Exposure&) = delete;

	uint32_t n_images() const { return nrs_exposure_n_images(m_exp); }
	// the values from the host ([n_images][3], or nullptr for zeros); the per-frame reset_state of the reference: moments, step count and cells start again
	void set(const float* h_values) { check(nrs_exposure_set(m_exp, h_values), "nrs_exposure_set"); }
	void get(nrs_exposure_what which, void* h_out) { check(nrs_exposure_get(m_exp, which, h_out, (size_t)3 * n_images()), "nrs_exposure_get"); }
	void export_values(float* d_out, void* stream) { check(nrs_exposure_export(m_exp, d_out, stream), "nrs_exposure_export"); }
	// per ray slot: the target scaled by its image's 2^exposure (for NerfNetwork::ray_loss_ex, in place of a gather) and the scale (for accumulate)
	void targets(void* stream, uint32_t n_rays, const uint32_t* d_ray_counter, const uint32_t* d_ray_indices, const uint32_t* d_pixels, const float* d_target_rgba,
	             float* d_target_out, uint32_t* d_scale) {
		check(nrs_exposure_targets(m_exp, stream, n_rays, d_ray_counter, d_ray_indices, d_pixels, d_target_rgba, d_target_out, d_scale), "nrs_exposure_targets");
	}
	void accumulate(void* stream, const nrs_exposure_accumulate_params& params, uint32_t n_rays, const uint32_t* d_ray_counter, const uint32_t* d_ray_indices,
	                const uint32_t* d_numsteps_out, const uint32_t* d_ray_aux, const uint32_t* d_scale, const float* d_xy_pdf) {
		check(nrs_exposure_accumulate(m_exp, stream, &params, n_rays, d_ray_counter, d_ray_indices, d_numsteps_out, d_ray_aux, d_scale, d_xy_pdf), "nrs_exposure_accumulate");
	}
	// every n_steps_between_cam_updates training steps
	void step(void* stream, float loss_scale, float learning_rate) { check(nrs_exposure_step(m_exp, stream, loss_scale, learning_rate), "nrs_exposure_step"); }
	uint32_t step() const { return nrs_exposure_step_count(m_exp); }
	nrs_exposure* get() const { return m_exp; }

private:
	nrs_exposure* m_exp = nullptr;
};

// nrs_image_metrics on a caller's reference (d_reference: fp16 or f32 RGBA, linear, premultiplied), and run.py's totals over records that are back on the host
inline void image_metrics(Context& ctx, void* stream, uint32_t width, uint32_t height, const float* d_image, const void* d_reference, nrs_image_format reference_format,
                          nrs_image_metrics_result* d_result, nrs_color_space color_space = NRS_COLOR_LINEAR, const float* background_rgba = nullptr, float* d_ssim_map = nullptr,
                          float* d_sq_err_map = nullptr) {
	const nrs_image_metrics_params p = image_metrics_params(color_space, background_rgba, reference_format);
	check(nrs_image_metrics(ctx.get(), stream, width, height, d_image, d_reference, &p, d_result, d_ssim_map, d_sq_err_map), "nrs_image_metrics");
}
inline nrs_metrics_summary metrics_summary(const nrs_image_metrics_result* h_results, uint32_t n) {
	nrs_metrics_summary s{};
	check(nrs_image_metrics_summary_host(h_results, n, &s), "nrs_image_metrics_summary_host");
	return s;
}

// EditOperator (edit_operator.h:43-91): the interface NerfTracer::m_edit_operators holds (testbed.h:237) -- cage deformations and affine
// duplications alike.  An operator owns its device tables.
class EditOperator {
public:
	virtual ~EditOperator() { nrs_edit_destroy(m_edit); }
	EditOperator(const EditOperator&) = delete;
	EditOperator& operator=(const EditOperator&) = delete;

	void map_rays(void* stream, float* d_nerf_coords /*[n x 7]*/, uint8_t* d_empty_mask, uint32_t n_elements) const {
		check(nrs_edit_map_rays(m_edit, stream, n_elements, d_nerf_coords, d_empty_mask), "nrs_edit_map_rays");
	}
	void map_positions(void* stream, float* d_nerf_pos, uint32_t stride_floats, uint8_t* d_empty_mask, uint32_t n_elements) const {
		check(nrs_edit_map_positions(m_edit, stream, n_elements, d_nerf_pos, stride_floats, d_empty_mask), "nrs_edit_map_positions");
	}
	nrs_edit* get() const { return m_edit; }

protected:
	EditOperator() = default;
	nrs_edit* m_edit = nullptr;
};

class CageDeformation : public EditOperator {
public:
	CageDeformation(Context& ctx, const nrs_model_desc& desc, const nrs_tet_mesh& mesh) { check(nrs_edit_create(ctx.get(), &desc, &mesh, &m_edit), "nrs_edit_create"); }
	// The per-gizmo-move chain (Cage::interpolate_with_mvc -> TetMesh::post_update_vertices -> build_tet_grid ->
	// update_local_rotations), on the device.  set_mvc once after Cage::compute_mvc; update_cage per move.
	void set_mvc(const float* h_weights, uint32_t n_cage_vertices) { check(nrs_edit_set_mvc(m_edit, h_weights, n_cage_vertices), "nrs_edit_set_mvc"); }
	void update_cage(void* stream, const float* h_cage_vertices, uint32_t n_cage_vertices) {
		check(nrs_edit_update_cage(m_edit, stream, h_cage_vertices, n_cage_vertices), "nrs_edit_update_cage");
	}
	void update_vertices(void* stream, const float* h_vertices, uint32_t n_vertices) {
		check(nrs_edit_update_vertices(m_edit, stream, h_vertices, n_vertices), "nrs_edit_update_vertices");
	}
	// GrowingSelection::interpolate_poisson_boundary (growing_selection.cu:2350): cage-vertex membrane terms -> the operator's per-tet-vertex ones;
	// h_gamma = TetMesh::gamma_coordinates or nullptr for the weights given to set_mvc
	void interpolate_poisson_boundary(void* stream, const float* h_gamma, uint32_t n_cage_vertices, const float* h_inside_density, const float* h_outside_density,
	                                  const float* h_inside_shs, const float* h_outside_shs, float residual_amplitude) {
		check(nrs_edit_poisson_interpolate(m_edit, stream, h_gamma, n_cage_vertices, h_inside_density, h_outside_density, h_inside_shs, h_outside_shs, residual_amplitude),
		      "nrs_edit_poisson_interpolate");
	}
};

class AffineDuplication : public EditOperator { // editing/affine_duplication.h:23-106
public:
	AffineDuplication(Context& ctx, const nrs_model_desc& desc, const nrs_affine_duplication& op) {
		check(nrs_edit_create_affine(ctx.get(), &desc, &op, &m_edit), "nrs_edit_create_affine");
	}
};

// View over the caller's frame / depth device arrays (CudaRenderBuffer::frame_buffer() / depth_buffer() / spp()).
struct RenderBuffer {
	float* frame_buffer;   // float4 [H*W], premultiplied linear RGBA; the caller clears it (clear_frame, testbed.cu:2635)
	float* depth_buffer;   // float [H*W]
	int width, height;     // in_resolution()
	uint32_t spp;          // sample index of this frame
	float* accumulate_buffer = nullptr; // float4 [H*W], optional: CudaRenderBuffer::m_accumulate_buffer
	// void CudaRenderBuffer::accumulate(float exposure, cudaStream_t stream) -- render_buffer.cu:540-560 (exposure is unused there too): the running mean of the spp frames
	void accumulate(Context& ctx, void* stream, nrs_color_space color_space = NRS_COLOR_LINEAR) {
		if (!accumulate_buffer) throw std::runtime_error("RenderBuffer::accumulate: no accumulate buffer");
		check(nrs_accumulate(ctx.get(), stream, (uint32_t)width, (uint32_t)height, frame_buffer, accumulate_buffer, spp, (uint32_t)color_space), "nrs_accumulate");
		++spp;
	}
	// m_color_space / m_tonemap_curve and their setters (render_buffer.h:226-238): a change resets the accumulation, as there
	nrs_color_space color_space = NRS_COLOR_LINEAR;
	nrs_tonemap_curve tonemap_curve = NRS_TONEMAP_IDENTITY;
	void set_color_space(nrs_color_space v) {
		if (v != color_space) { color_space = v; spp = 0; }
	}
	void set_tonemap_curve(nrs_tonemap_curve v) {
		if (v != tonemap_curve) { tonemap_curve = v; spp = 0; }
	}
	// void CudaRenderBuffer::tonemap(float exposure, const Array4f& background_color, EColorSpace output_color_space, cudaStream_t stream, Vector4f* lopi) -- render_buffer.h:205,
	// render_buffer.cu:562-580.  The reference writes its surface (and lopi); here the caller names the output: d_out [H*W] f32x4 (NRS_TONEMAP_RGBA32F; may be the accumulate
	// buffer itself) or one R, G, B, A dword per pixel (NRS_TONEMAP_RGBA8).  Reads the accumulate buffer in m_color_space.
	void tonemap(Context& ctx, float exposure, const float background_color[4], nrs_color_space output_color_space, void* stream, void* d_out,
	             uint32_t output_format = NRS_TONEMAP_RGBA32F, bool clamp_output_color = false) {
		if (!accumulate_buffer) throw std::runtime_error("RenderBuffer::tonemap: no accumulate buffer");
		nrs_tonemap_params t{};
		t.struct_size = (uint32_t)sizeof(nrs_tonemap_params);
		t.exposure = exposure;
		for (int i = 0; i < 4; ++i) t.background_color[i] = background_color[i];
		t.color_space = (uint32_t)color_space;
		t.output_color_space = (uint32_t)output_color_space;
		t.tonemap_curve = (uint32_t)tonemap_curve;
		t.clamp_output = clamp_output_color ? 1u : 0u;
		t.output_format = output_format;
		check(nrs_tonemap(ctx.get(), stream, (uint32_t)width, (uint32_t)height, accumulate_buffer, &t, d_out), "nrs_tonemap");
	}
};

// The slice of ngp::Testbed that render_nerf reads (SURVEY 8b "implicit inputs"), with the reference's member names.
class Testbed {
public:
	struct Nerf {
		float cone_angle_constant = 0.f;            // 0 for aabb_scale 1, 1/256 otherwise (testbed_nerf.cu:3410-3425)
		float rendering_min_transmittance = 0.01f;
		bool training_linear_colors = false;
		float light_dir[3] = {0.5f, 0.5f, 0.5f};    // testbed.h:639; render_nerf passes light_dir.normalized() to every sample of a network with extra dims (:3135)
	} m_nerf;
	float m_render_aabb_min[3] = {0, 0, 0}, m_render_aabb_max[3] = {1, 1, 1};
	bool m_snap_to_pixel_centers = true;
	bool m_enable_edits = true;
	nrs_render_mode m_render_mode = NRS_RENDER_SHADE;
	int m_visualized_layer = 0, m_visualized_dimension = -1; // testbed.h: > -1 selects render mode EncodingVis (testbed_nerf.cu:3072)
	std::vector<const EditOperator*> m_edit_operators; // NerfTracer::m_edit_operators (testbed.h:237), applied last-to-first
	bool m_poisson_target = true;                     // NerfTracer::m_poisson_target (testbed.h:219: true, its checkbox is commented out; passed to composite_kernel_nerf, testbed_nerf.cu:2983)
	int m_show_accel = -1;                            // m_nerf.show_accel: >= 0 forces that cascade as the minimum while marching (:2751, :2849), makes
	                                                  // every sample opaque (:788-790) and colours the occupancy cells in render mode Positions (:911-920)
	float m_dof = 0.f;                                // aperture of pixel_to_ray's thin-lens branch (common_device.cuh:285-293)
	float m_slice_plane_z = 0.f, m_scale = 1.f;       // plane_z = m_slice_plane_z + m_scale (testbed_nerf.cu:3067): focus distance / slice plane
	float m_dataset_scale = 1.f;                      // m_nerf.training.dataset.scale: depth_scale = 1 / it (:3113)
	// camera model and background (render_nerf passes them to init_rays_from_camera, :3078-3100).  Device pointers, owned by the caller.
	uint32_t m_render_distortion_mode = 0;            // m_nerf.render_distortion.mode when m_nerf.render_with_camera_distortion (ECameraDistortionMode)
	float m_render_distortion_params[7] = {};         // m_nerf.render_distortion.params
	const float* m_distortion_map = nullptr;          // m_distortion.map->params_inference() (float2 [res.y][res.x]) when render_with_camera_distortion, else NULL
	int m_distortion_resolution[2] = {0, 0};          // m_distortion.resolution
	const float* m_envmap = nullptr;                  // m_envmap.envmap->params_inference() (float RGBA [res.y][res.x]), NULL when the snapshot has none
	int m_envmap_resolution[2] = {0, 0};              // m_envmap.resolution
	int m_glow_mode = 0;                              // m_nerf.m_glow_mode, m_nerf.m_glow_y_cutoff: composite_kernel_nerf's grid / cut-line overlay (:806-903)
	float m_glow_y_cutoff = 0.f;

	// Testbed state update_density_grid_nerf_operator advances: m_rng, m_nerf.density_grid_ema_step, density_grid_decay, max_cascade
	nrs_grid_update m_density_grid_update{};
	void seed_density_grid_update(uint32_t max_cascade, uint64_t seed = 1337, float decay = 0.95f) {
		m_density_grid_update = nrs_grid_update{};
		m_density_grid_update.n_uniform_samples = NRS_GRID_VOLUME * (max_cascade + 1);
		m_density_grid_update.max_cascade = max_cascade;
		m_density_grid_update.decay = decay;
		nrs_rng_seed(seed, &m_density_grid_update.rng_state, &m_density_grid_update.rng_inc);
	}
	// void Testbed::update_density_grid_nerf_render(uint32_t n_iterations, bool reset_grid, cudaStream_t)  -- testbed_nerf.cu:3514
	void update_density_grid_nerf_render(NerfNetwork& network, uint32_t n_iterations, bool reset_grid, void* stream) {
		std::vector<nrs_edit*> edits;
		if (m_enable_edits) for (const EditOperator* op : m_edit_operators) edits.push_back(op->get());
		for (uint32_t i = 0; i < n_iterations; ++i) {
			m_density_grid_update.reset_grid = (reset_grid && i == 0) ? 1u : 0u;
			check(nrs_model_update_density_grid(network.get(), edits.data(), (int)edits.size(), &m_density_grid_update, stream),
			      "nrs_model_update_density_grid");
		}
		m_density_grid_update.reset_grid = 0;
	}

	// the nrs_render_params of a frame of this testbed: what render_nerf and render_to_cpu hand to the library
	nrs_render_params make_params(int width, int height, uint32_t spp_index, const float focal_length[2], const float camera_matrix0[12], const float camera_matrix1[12],
	                              const float rolling_shutter[4], const float screen_center[2], bool apply_operators) const {
		nrs_render_params p{}; // = NRS_RENDER_PARAMS_INIT, spelled so that -Wextra stays quiet in C++
		p.struct_size = (uint32_t)sizeof(nrs_render_params);
		p.resolution[0] = width;
		p.resolution[1] = height;
		for (int i = 0; i < 2; ++i) { p.focal_length[i] = focal_length[i]; p.screen_center[i] = screen_center[i]; }
		for (int i = 0; i < 12; ++i) { p.camera_matrix0[i] = camera_matrix0[i]; p.camera_matrix1[i] = camera_matrix1[i]; }
		for (int i = 0; i < 4; ++i) p.rolling_shutter[i] = rolling_shutter[i];
		for (int i = 0; i < 3; ++i) { p.render_aabb_min[i] = m_render_aabb_min[i]; p.render_aabb_max[i] = m_render_aabb_max[i]; }
		p.spp_index = spp_index;
		p.snap_to_pixel_centers = m_snap_to_pixel_centers;
		p.min_transmittance = m_nerf.rendering_min_transmittance;
		p.cone_angle_constant = m_nerf.cone_angle_constant;
		p.render_mode = m_visualized_dimension > -1 ? (uint32_t)NRS_RENDER_ENCODING_VIS : (uint32_t)m_render_mode; // testbed_nerf.cu:3072
		p.visualized_layer = (uint32_t)m_visualized_layer;
		p.visualized_dimension = m_visualized_dimension > -1 ? (uint32_t)m_visualized_dimension : 0u;
		p.linear_colors = m_nerf.training_linear_colors;
		p.apply_operators = apply_operators && m_enable_edits;
		p.poisson_target = m_poisson_target ? 1u : 0u;
		p.min_mip = m_show_accel >= 0 ? (uint32_t)m_show_accel : 0u;
		p.show_accel = m_show_accel >= 0 ? 1u : 0u;
		p.dof = m_dof;
		p.slice_plane_z = m_slice_plane_z + m_scale;
		p.depth_scale = 1.0f / m_dataset_scale;
		p.distortion_mode = m_render_distortion_mode;
		for (int i = 0; i < 7; ++i) p.distortion_params[i] = m_render_distortion_params[i];
		p.d_distortion_map = m_distortion_map;
		p.d_envmap = m_envmap;
		p.glow_mode = (uint32_t)m_glow_mode;
		p.glow_y_cutoff = m_glow_y_cutoff;
		for (int i = 0; i < 2; ++i) { p.distortion_resolution[i] = m_distortion_resolution[i]; p.envmap_resolution[i] = m_envmap_resolution[i]; }
		return p;
	}

	// void Testbed::render_nerf(NerfNetwork<precision_t>&, CudaRenderBuffer&, const Vector2i& max_res, const Vector2f& focal_length,
	//     const Matrix<float,3,4>& camera_matrix0, const Matrix<float,3,4>& camera_matrix1, const Vector4f& rolling_shutter,
	//     const Vector2f& screen_center, bool apply_operators, cudaStream_t stream)              -- testbed.h:305
	void render_nerf(NerfNetwork& network, RenderBuffer& render_buffer, const int /*max_res*/[2], const float focal_length[2],
	                 const float camera_matrix0[12], const float camera_matrix1[12], const float rolling_shutter[4], const float screen_center[2],
	                 bool apply_operators, void* stream, nrs_render_stats* stats = nullptr) {
		const nrs_render_params p = make_params(render_buffer.width, render_buffer.height, render_buffer.spp, focal_length, camera_matrix0, camera_matrix1, rolling_shutter,
		                                        screen_center, apply_operators);
		check(nrs_model_set_light_dir(network.get(), m_nerf.light_dir), "nrs_model_set_light_dir"); // (no effect on a network without extra dims)
		std::vector<nrs_edit*> edits;
		for (const EditOperator* op : m_edit_operators) edits.push_back(op->get());
		check(nrs_render_nerf(network.get(), &p, edits.data(), (int)edits.size(), render_buffer.frame_buffer, render_buffer.depth_buffer, nullptr, stream,
		                      stats),
		      "nrs_render_nerf");
	}

	// ---- mesh extraction (src/testbed_nerf.cu:4614-4649, src/testbed.cu:337-343, src/marching_cubes.cu:48-55) ----
	// m_mesh: the device-resident mesh of the last marching_cubes call (verts, vert_normals, vert_colors, verts_smoothed, indices behind nrs_mesh_device)
	struct Mesh {
		float thresh = 2.5f;           // m_mesh.thresh
		nrs_mesh* handle = nullptr;
		Mesh() = default;
		Mesh(const Mesh&) = delete;
		Mesh& operator=(const Mesh&) = delete;
		~Mesh() { nrs_mesh_destroy(handle); }
	} m_mesh;
	float m_dataset_offset[3] = {0.f, 0.f, 0.f};      // m_nerf.training.dataset.offset (save_mesh writes (v - offset) / scale)
	// Vector3i get_marching_cubes_res(uint32_t res_1d, const BoundingBox& aabb)
	static void get_marching_cubes_res(uint32_t res_1d, const float aabb_min[3], const float aabb_max[3], int res3d_out[3]) {
		uint32_t r[3];
		check(nrs_marching_cubes_res(res_1d, aabb_min, aabb_max, r), "nrs_marching_cubes_res");
		for (int i = 0; i < 3; ++i) res3d_out[i] = (int)r[i];
	}
	// int Testbed::marching_cubes(Vector3i res3d, const BoundingBox& aabb, float thresh): thresh == FLT_MAX means m_mesh.thresh; returns the number of triangles
	int marching_cubes(NerfNetwork& network, const int res3d[3], const float aabb_min[3], const float aabb_max[3], float thresh, void* stream = nullptr) {
		if (res3d[0] < 0 || res3d[1] < 0 || res3d[2] < 0) throw std::runtime_error("Testbed::marching_cubes: negative resolution");
		if (thresh == 3.402823466e+38f) thresh = m_mesh.thresh;
		const uint32_t r[3] = {(uint32_t)res3d[0], (uint32_t)res3d[1], (uint32_t)res3d[2]};
		check(nrs_model_set_light_dir(network.get(), m_nerf.light_dir), "nrs_model_set_light_dir");
		nrs_mesh* mesh = nullptr;
		check(nrs_mesh_extract(network.get(), stream, r, aabb_min, aabb_max, thresh, 1, m_nerf.training_linear_colors ? 1 : 0, &mesh), "nrs_mesh_extract");
		nrs_mesh_destroy(m_mesh.handle);
		m_mesh.handle = mesh;
		uint32_t n_tris = 0;
		check(nrs_mesh_counts(mesh, nullptr, nullptr, &n_tris), "nrs_mesh_counts");
		return (int)n_tris;
	}
	// void Testbed::compute_and_save_marching_cubes_mesh(const char* filename, Vector3i res3d, BoundingBox aabb, float thresh, bool unwrap_it): an empty box (NULL) is the render box
	void compute_and_save_marching_cubes_mesh(NerfNetwork& network, const char* filename, const int res3d[3], const float* aabb_min = nullptr, const float* aabb_max = nullptr,
	                                          float thresh = 2.5f, bool unwrap_it = false) {
		if (unwrap_it) throw std::runtime_error("Testbed::compute_and_save_marching_cubes_mesh: unwrap_it (the UV unwrap and its texture) is not built");
		const bool empty = !aabb_min || !aabb_max;
		marching_cubes(network, res3d, empty ? m_render_aabb_min : aabb_min, empty ? m_render_aabb_max : aabb_max, thresh);
		uint32_t n_padded = 0, n_tris = 0;
		check(nrs_mesh_counts(m_mesh.handle, nullptr, &n_padded, &n_tris), "nrs_mesh_counts");
		std::vector<float> verts((size_t)n_padded * 3), normals((size_t)n_padded * 3), colors((size_t)n_padded * 3);
		std::vector<uint32_t> indices((size_t)n_tris * 3);
		check(nrs_mesh_download(m_mesh.handle, verts.data(), normals.data(), colors.data(), nullptr, indices.data()), "nrs_mesh_download");
		check(nrs_mesh_write(filename, n_padded, verts.data(), normals.data(), colors.data(), n_tris, indices.data(), m_dataset_scale, m_dataset_offset), "nrs_mesh_write");
	}

	// ---- Testbed::render_to_cpu and the camera state it moves (src/python_api.cu:129-175, src/testbed.cu:2086-2111) ----
	// m_windowless_render_surface: device arrays of the caller.  `frames` / `depths` hold n_slabs slabs, slab_stride_pixels apart (>= width * height), one per sample of a
	// launch; the tonemapped image is left in d_out (nrs_tonemap_output_bytes) for the caller to copy to the host, where the reference copies its surface.
	struct WindowlessSurface {
		int width = 0, height = 0;
		float* frames = nullptr;             // float4 [n_slabs][slab_stride_pixels]; the caller clears them (clear_frame, testbed.cu:2635)
		float* depths = nullptr;             // float  [n_slabs][slab_stride_pixels]
		size_t slab_stride_pixels = 0;
		uint32_t n_slabs = 0;                // samples per launch: 1 .. NRS_SPP_BATCH_MAX
		float* accumulate_buffer = nullptr;  // float4 [H*W]
		void* d_out = nullptr;
		uint32_t output_format = NRS_TONEMAP_RGBA32F;
		nrs_color_space color_space = NRS_COLOR_LINEAR;
		nrs_tonemap_curve tonemap_curve = NRS_TONEMAP_IDENTITY;
		// clears the slabs before a launch.  Null: the caller's own device memset is not available to this header, so render_to_cpu refuses more than one batch per call
		void (*clear_slabs)(WindowlessSurface&, void* stream) = nullptr;
	};
	float m_camera[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};          // m_camera, 3x4 column-major
	float m_smoothed_camera[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0}; // m_smoothed_camera: the camera the last frame ended on
	bool m_camera_smoothing = false;
	float m_fov = 50.625f;                                              // fov() in degrees, along m_fov_axis
	int m_fov_axis = 1;
	float m_screen_center[2] = {0.5f, 0.5f};
	float m_exposure = 0.f;
	float m_background_color[4] = {0, 0, 0, 0};
	std::vector<nrs_camera_keyframe> m_camera_path;                     // m_camera_path.m_keyframes

	// Testbed::load_camera_path -> CameraPath::load (src/camera_path.cu:114-136)
	void load_camera_path(const char* path) {
		nrs_camera_path* h = nullptr;
		check(nrs_camera_path_open(path, &h), "nrs_camera_path_open");
		m_camera_path.assign(nrs_camera_path_count(h), nrs_camera_keyframe{});
		const int st = nrs_camera_path_keyframes(h, m_camera_path.data(), (uint32_t)m_camera_path.size());
		nrs_camera_path_close(h);
		check(st, "nrs_camera_path_keyframes");
	}
	// void Testbed::set_camera_from_time(float t) -- src/testbed.cu:2099-2111: nothing without keyframes
	void set_camera_from_time(float t) {
		if (m_camera_path.empty()) return;
		nrs_camera_keyframe k{};
		check(nrs_camera_path_eval(m_camera_path.data(), (uint32_t)m_camera_path.size(), t, &k), "nrs_camera_path_eval");
		check(nrs_camera_keyframe_matrix(&k, m_camera), "nrs_camera_keyframe_matrix");
		m_slice_plane_z = k.slice; m_scale = k.scale; m_fov = k.fov; m_dof = k.dof;
	}
	// void Testbed::apply_camera_smoothing(float elapsed_ms) -- src/testbed.cu:2086-2093
	void apply_camera_smoothing(float elapsed_ms) {
		if (m_camera_smoothing) {
			const float decay = std::pow(0.02f, elapsed_ms / 1000.0f);
			float out[12];
			check(nrs_log_space_lerp(m_smoothed_camera, m_camera, 1.0f - decay, out), "nrs_log_space_lerp");
			for (int i = 0; i < 12; ++i) m_smoothed_camera[i] = out[i];
		} else {
			for (int i = 0; i < 12; ++i) m_smoothed_camera[i] = m_camera[i];
		}
	}
	// Testbed::calc_focal_length (src/testbed.cu:2556) with zoom 1: fov_to_focal_length(resolution[m_fov_axis], fov), evaluated as nrs_motion_views does
	void calc_focal_length(int width, int height, float out[2]) const {
		const double rel = 0.5 / std::tan(0.5 * (double)m_fov * 3.14159265358979323846 / 180.0);
		out[0] = out[1] = (float)(rel * (double)(m_fov_axis == 0 ? width : height));
	}

	// py::array_t<float> Testbed::render_to_cpu(int width, int height, int spp, bool linear, float start_time, float end_time, float fps, float shutter_fraction)
	//     -- src/python_api.cu:129-175.  The accumulation is reset; with start_time >= 0 the frame runs from m_smoothed_camera to the (smoothed) camera of end_time and every
	// sample renders between its own two cameras, with the path's fov / dof / focus plane at its own time (nrs_motion_views), a view per sample and one launch per
	// surface.n_slabs samples (nrs_render_nerf_spp_views); with start_time < 0 every sample renders m_camera (nrs_render_nerf_spp).  The slabs are folded into the running
	// mean and the last fold is fused with the display step (m_exposure, m_background_color; sRGB unless `linear`).  m_smoothed_camera is left at the end camera.
	// m_autofocus is not mirrored.  Not synchronised: the image is in surface.d_out once `stream` has run.
	void render_to_cpu(Context& ctx, NerfNetwork& network, WindowlessSurface& surface, int spp, bool linear, float start_time = -1.f, float end_time = -1.f, float fps = 30.f,
	                   float shutter_fraction = 1.0f, void* stream = nullptr, nrs_render_stats* stats = nullptr) {
		if (spp < 1) throw std::runtime_error("Testbed::render_to_cpu: spp must be at least 1");
		if (!surface.frames || !surface.depths || !surface.accumulate_buffer || !surface.d_out || surface.n_slabs == 0u || surface.n_slabs > NRS_SPP_BATCH_MAX)
			throw std::runtime_error("Testbed::render_to_cpu: the surface needs frames, depths, an accumulate buffer, d_out and 1 .. NRS_SPP_BATCH_MAX slabs");
		if ((uint32_t)spp > surface.n_slabs && !surface.clear_slabs)
			throw std::runtime_error("Testbed::render_to_cpu: spp above the surface's slabs needs surface.clear_slabs between the launches");
		if (end_time < 0.f) end_time = start_time;
		float start_cam[12], end_cam[12];
		for (int i = 0; i < 12; ++i) start_cam[i] = m_smoothed_camera[i];
		if (start_time >= 0.f) {
			set_camera_from_time(end_time);
			apply_camera_smoothing(1000.f / fps);
		} else {
			for (int i = 0; i < 12; ++i) start_cam[i] = m_smoothed_camera[i] = m_camera[i];
		}
		for (int i = 0; i < 12; ++i) end_cam[i] = m_smoothed_camera[i];
		const float rolling_shutter[4] = {0.f, 0.f, 0.f, 0.f};
		nrs_sample_view base{};
		calc_focal_length(surface.width, surface.height, base.focal_length);
		base.dof = m_dof;
		base.slice_plane_z = m_slice_plane_z + m_scale;
		const int32_t resolution[2] = {surface.width, surface.height};
		std::vector<nrs_edit*> edits;
		for (const EditOperator* op : m_edit_operators) edits.push_back(op->get());
		check(nrs_model_set_light_dir(network.get(), m_nerf.light_dir), "nrs_model_set_light_dir");
		nrs_tonemap_params t{};
		t.struct_size = (uint32_t)sizeof(nrs_tonemap_params);
		t.exposure = m_exposure;
		for (int i = 0; i < 4; ++i) t.background_color[i] = m_background_color[i];
		t.color_space = (uint32_t)surface.color_space;
		t.output_color_space = linear ? 0u : 1u;
		t.tonemap_curve = (uint32_t)surface.tonemap_curve;
		t.output_format = surface.output_format;
		if (stats) *stats = nrs_render_stats{};
		std::vector<nrs_sample_view> views(surface.n_slabs);
		for (uint32_t done = 0; done < (uint32_t)spp;) {
			const uint32_t k = (uint32_t)spp - done < surface.n_slabs ? (uint32_t)spp - done : surface.n_slabs;
			if (done != 0u) surface.clear_slabs(surface, stream);
			const bool moving = start_time >= 0.f;
			if (moving)
				check(nrs_motion_views(start_cam, end_cam, shutter_fraction, k, done, (uint32_t)spp, resolution, m_fov_axis, m_camera_path.data(), (uint32_t)m_camera_path.size(),
				                       start_time, end_time, &base, views.data()), "nrs_motion_views");
			const nrs_render_params p = make_params(surface.width, surface.height, done, base.focal_length, moving ? views[0].camera_matrix0 : start_cam,
			                                        moving ? views[0].camera_matrix1 : end_cam, rolling_shutter, m_screen_center, true);
			nrs_render_stats batch_stats{};
			check(nrs_render_nerf_spp_views(network.get(), &p, edits.data(), (int)edits.size(), k, moving ? views.data() : nullptr, surface.frames, surface.depths, nullptr,
			                                surface.slab_stride_pixels, stream, stats ? &batch_stats : nullptr), "nrs_render_nerf_spp_views");
			if (stats) { stats->n_samples += batch_stats.n_samples; stats->n_rays_alive += batch_stats.n_rays_alive; stats->n_rays_hit += batch_stats.n_rays_hit; }
			if (done + k < (uint32_t)spp)
				check(nrs_accumulate_spp(ctx.get(), stream, (uint32_t)surface.width, (uint32_t)surface.height, surface.frames, surface.slab_stride_pixels, k, surface.accumulate_buffer,
				                         done, (uint32_t)surface.color_space), "nrs_accumulate_spp");
			else
				check(nrs_accumulate_spp_tonemap(ctx.get(), stream, (uint32_t)surface.width, (uint32_t)surface.height, surface.frames, surface.slab_stride_pixels, k,
				                                 surface.accumulate_buffer, done, &t, surface.d_out), "nrs_accumulate_spp_tonemap");
			done += k;
		}
		if (start_time >= 0.f) { // the loop's last set_camera_from_time (:156): the testbed is left on the last sample's keyframe
			const float a0 = ((float)(spp - 1)) / (float)spp * shutter_fraction, a1 = ((float)(spp - 1) + 1.0f) / (float)spp * shutter_fraction;
			set_camera_from_time(start_time + (end_time - start_time) * (a0 + a1) / 2.0f);
		}
		for (int i = 0; i < 12; ++i) m_smoothed_camera[i] = end_cam[i]; // :167-168
	}
};

// GrowingSelection's growing and fine-mesh members (editing/tools/growing_selection.h; RegionGrowing, region_growing.h): thin forwards to the nrs_selection_* calls.
// The context is needed by dilate, erode and extract_fine_mesh only (NULL: a host-only selection).
class GrowingSelection {
public:
	GrowingSelection(nrs_ctx* ctx, const std::vector<float>& density_grid, uint32_t max_cascade) : m_ctx(ctx) {
		check(nrs_selection_create(density_grid.data(), density_grid.size(), max_cascade, &m_sel), "nrs_selection_create");
	}
	~GrowingSelection() {
		nrs_mesh_destroy(m_selection_mesh);
		nrs_selection_destroy(m_sel);
	}
	GrowingSelection(const GrowingSelection&) = delete;
	GrowingSelection& operator=(const GrowingSelection&) = delete;
	nrs_selection* get() const { return m_sel; }

	bool m_use_morphological = true;
	float m_density_threshold = 0.01f;
	int m_growing_steps = 10000;
	nrs_mesh* m_selection_mesh = nullptr; // selection_mesh of the last extract_fine_mesh, on the device

	void reset_growing(const std::vector<uint32_t>& selected_cells, int growing_level) {
		check(nrs_selection_reset(m_sel, selected_cells.data(), (uint32_t)selected_cells.size(), (uint32_t)growing_level), "nrs_selection_reset");
	}
	// grow_region(density_threshold, ERegionGrowingMode::Manual, growing_level, growing_steps); returns the entries popped
	uint32_t grow_region(float density_threshold, int growing_level, int growing_steps) {
		uint32_t popped = 0;
		check(nrs_selection_grow(m_sel, density_threshold, (uint32_t)growing_level, growing_steps < 0 ? 0u : (uint32_t)growing_steps, &popped), "nrs_selection_grow");
		return popped;
	}
	void upscale_growing() { check(nrs_selection_upscale(m_sel), "nrs_selection_upscale"); }
	void dilate(void* stream = nullptr) { check(nrs_selection_dilate(m_ctx, stream, m_sel), "nrs_selection_dilate"); }
	void erode(void* stream = nullptr) { check(nrs_selection_erode(m_ctx, stream, m_sel), "nrs_selection_erode"); }
	void extract_fine_mesh(void* stream = nullptr) {
		nrs_mesh* mesh = nullptr;
		check(nrs_selection_fine_mesh(m_ctx, stream, m_sel, m_use_morphological ? 1 : 0, &mesh), "nrs_selection_fine_mesh");
		nrs_mesh_destroy(m_selection_mesh);
		m_selection_mesh = mesh;
	}
	int growing_level() const {
		uint32_t level = 0;
		check(nrs_selection_state(m_sel, &level, nullptr, nullptr, nullptr), "nrs_selection_state");
		return (int)level;
	}
	std::vector<uint32_t> selection_cell_idx() const {
		uint32_t n = 0;
		check(nrs_selection_state(m_sel, nullptr, &n, nullptr, nullptr), "nrs_selection_state");
		std::vector<uint32_t> cells(n);
		check(nrs_selection_get_cells(m_sel, cells.data(), nullptr), "nrs_selection_get_cells");
		return cells;
	}
	std::vector<float> selection_points() const { // x, y, z per cell
		uint32_t n = 0;
		check(nrs_selection_state(m_sel, nullptr, &n, nullptr, nullptr), "nrs_selection_state");
		std::vector<float> points((size_t)n * 3);
		check(nrs_selection_get_cells(m_sel, nullptr, points.data()), "nrs_selection_get_cells");
		return points;
	}
	std::vector<uint8_t> selection_grid_bitfield() const {
		std::vector<uint8_t> bits(NRS_BITFIELD_BYTES);
		check(nrs_selection_get_bitfield(m_sel, bits.data()), "nrs_selection_get_bitfield");
		return bits;
	}

private:
	nrs_ctx* m_ctx = nullptr;
	nrs_selection* m_sel = nullptr;
};

} // namespace compat
} // namespace nrs
