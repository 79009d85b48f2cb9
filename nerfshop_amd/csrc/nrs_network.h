// nrs_network.h -- the launchers of nrs_network.hip: the network and the hash grid on caller batches, and the kernels built on them.
#pragma once
#include <stdint.h>
#include "../../include/nrs.h"
#include "nrs_internal.h"

namespace nrs {

int launch_trace_samples(const DeviceModel& m, const nrs_render_params& p, uint32_t n_pixels, const uint32_t* d_pixel_idx,
                         uint32_t max_samples, float* d_t, float* d_dt, uint32_t* d_count, void* stream);
// The operators of network_kernel on caller batches (its MODE template argument: an unscoped enum, so the kernels keep their `int` symbol names).
enum NetOp : int {
	kNetInference = 0,          // inference_mixed_precision: 16 channels, c3 = density raw
	kNetDensity = 1,            // density(): the density MLP's outputs
	kNetEncode = 2,             // the hash-grid features, fp16 [n x 32]
	kNetInputGradient = 3,      // input_gradient(stream, 3, ...): d density_raw / d position, f32 [n x 3]
	kNetVisualizeActivation = 4,// visualize_activation(vis_layer, vis_dim): f32 [n]
	kNetInferenceDeep = 5,      // kNetInference of a network with a third rgb hidden layer: the launcher's choice (DeviceModel::rgb_deep), never a caller's
};
// ld_out, layout: kNetInference / kNetDensity / kNetEncode only; vis_layer (a kernel layer: nrs_api_network.cpp kernel_layer), vis_dim: kNetVisualizeActivation only.
// per_sample_light: floats 7..9 of a record are that sample's warped light direction (a model with n_extra_dims = 3 and ld_in >= 10); else DeviceModel::light01
int launch_network(const DeviceModel& m, NetOp op, uint32_t n, const float* d_in, uint32_t ld_in, void* d_out, uint32_t ld_out,
                   int layout, int n_cus, void* stream, bool per_sample_light = false, uint32_t vis_layer = 0, uint32_t vis_dim = 0);
int launch_selection_rays(const DeviceModel& m, const nrs_render_params& p, const int32_t* d_pixels, uint32_t n, float threshold,
                          float* d_positions, uint32_t* d_cells, uint8_t* d_found, void* stream);
int launch_poisson_fit(const DeviceModel& m, uint32_t n_verts, uint32_t n_sh, const float* d_coords, const void* d_net, int is_inside, float scale,
                       float* d_density, float* d_sh, void* stream);
enum GridEvalOp : int { kGridDensity = 0, kGridRgba = 1 }; // get_density_on_grid / get_rgba_on_grid (grid_eval_kernel's MODE)
int launch_grid_eval(const DeviceModel& m, GridEvalOp op, const uint32_t res[3], const float box_mn[3], const float box_mx[3], const float dir01[3],
                     const float* d_density_grid, float* d_out, int n_cus, void* stream);

} // namespace nrs
