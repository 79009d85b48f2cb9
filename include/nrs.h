/*
 * nrs.h -- C-ABI of the MI355X-native NeRFshop render path ("nrs" = NeRFshop Render path, Standalone).
 *
 * This is the drop-in boundary for ONE hot path of graphdeco-inria/nerfshop: the volumetric render path
 * (occupancy-grid marching -> cage/tet warp of samples -> hash-grid encoding -> fused MLPs -> compositing).
 * The reference has no FFI for this path; it sits behind C++ members called from one host thread on one
 * stream.  Every entry point below names the reference interface it replaces (paths relative to the
 * reference checkout):
 *
 *   nrs_render_nerf          <- Testbed::render_nerf                   src/testbed_nerf.cu:3066 (decl testbed.h:305)
 *                               = NerfTracer::init_rays_from_camera    src/testbed_nerf.cu:2683
 *                               + NerfTracer::trace                    src/testbed_nerf.cu:2772
 *                               + shade_kernel_nerf                    src/testbed_nerf.cu:2448
 *   nrs_network_inference    <- NerfNetwork<T>::inference_mixed_precision   include/.../nerf_network_full.h:62
 *   nrs_network_density      <- NerfNetwork<T>::density                     include/.../nerf_network_full.h:223
 *   nrs_density_on_grid / nrs_rgba_on_grid <- Testbed::get_density_on_grid / get_rgba_on_grid   src/testbed_nerf.cu:4538 / :4588  ("next" row f4)
 *   nrs_model_set_params / _device <- NerfNetwork<T>::set_params            include/.../nerf_network_full.h:316 (host blob / device pointers)
 *   nrs_model_set_density_grid <- Testbed::update_density_grid_mean_and_bitfield   src/testbed_nerf.cu:3642
 *   nrs_edit_create          <- TetMesh GPU members + upload                       tet_mesh.h:80-94, tet_mesh.cu:651-667
 *   nrs_edit_update_cage / _vertices <- interpolate_with_mvc + build_tet_grid + update_local_rotations, on the device   ("next" row f1)
 *   nrs_edit_create_affine   <- AffineDuplication ctor + update_destination         editing/affine_duplication.h:26, :77   ("next" row f4)
 *   nrs_edit_map_rays        <- EditOperator::map_rays      edit_operator.h:43, CageDeformation::map_rays  cage_deformation.cu:547
 *   nrs_edit_map_positions   <- EditOperator::map_positions edit_operator.h:51, cage_deformation.cu:624
 *   nrs_edit_poisson_interpolate <- GrowingSelection::interpolate_poisson_boundary  src/editing/tools/growing_selection.cu:2350
 *   nrs_model_update_density_grid <- Testbed::update_density_grid_nerf_operator       src/testbed_nerf.cu:3533   ("next" row f2)
 *   nrs_snapshot_open        <- Testbed::load_snapshot / load_network_config        src/testbed.cu:3054 / :152       ("next" row f3)
 *   nrs_edits_open           <- Testbed::load_edits                                 src/testbed.cu:3205              ("next" row f3)
 *   nrs_tet_lut_build        <- TetMesh::build_tet_grid / build_original_tet_grid  tet_mesh.cu:368 / :76   (host, "next" row f1)
 *   nrs_mvc_compute / nrs_mvc_apply <- Cage::compute_mvc / interpolate_with_mvc    cage.cu:6 / :38          (host, "next" row f1)
 *   nrs_tet_local_rotations  <- TetMesh::update_local_rotations                    tet_mesh.cu:37           (host, "next" row f1)
 *   nrs_trace_samples        <- (test hook) the (t, dt) stream generate_next_nerf_network_inputs emits, testbed_nerf.cu:637
 *   nrs_accumulate           <- CudaRenderBuffer::accumulate / accumulate_kernel                                   src/render_buffer.cu:540 / :217
 *   nrs_tonemap              <- CudaRenderBuffer::tonemap / tonemap_kernel                                         src/render_buffer.cu:562 / :471
 *   nrs_detile               <- (new) inverse of the multi-GPU tile packing, no reference counterpart
 *   nrs_mesh_extract / nrs_mesh_from_density / nrs_mesh_write <- Testbed::marching_cubes src/testbed_nerf.cu:4614, marching_cubes_gpu / save_mesh src/marching_cubes.cu:730 / :760
 *   nrs_dataset_rays         <- generate_training_samples_nerf up to the ray   src/testbed_nerf.cu:1087-1186, and the target / background look-ups of :1777-1806
 *   nrs_dataset_set_image    <- from_rgba32 / from_fullp                       common_device.cuh:513, src/nerf_loader.cu:62
 *   nrs_dataset_mark_untrained <- mark_untrained_density_grid                  src/testbed_nerf.cu:353
 *
 * Conventions: every function returns NRS_OK (0) or a negative nrs_status; nrs_last_error() returns a
 * thread-local message.  All buffers named d_* are DEVICE pointers owned by the caller; h_* are HOST
 * pointers.  `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls are asynchronous
 * on `stream` unless stated; the caller synchronises (the reference does the same, src/testbed.cu:2843).
 * A context is not thread-safe; use one per host thread / GPU.  Render calls issued back to back on DIFFERENT streams may
 * overlap on the device (double-buffered frames; up to 8 in flight per context).  No torch / C++ types cross this boundary.
 */
#ifndef NRS_H
#define NRS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NRS_ABI_VERSION 3   /* 3: nrs_render_params starts with struct_size (every entry point that takes the struct refuses a size other than its own: a client
                             * built against another header is turned away instead of being read past its struct); visualized_layer / _dimension appended.
                             * 2: dof / slice_plane_z / depth_scale / show_accel, camera model, background, glow */

typedef enum nrs_status {
	NRS_OK = 0,
	NRS_ERR_INVALID_ARG = -1,
	NRS_ERR_UNSUPPORTED = -2,   /* configuration outside configs/nerf/base.json's architecture */
	NRS_ERR_HIP = -3,           /* a HIP runtime call failed; message carries hipGetErrorString */
	NRS_ERR_NO_DEVICE = -4,     /* no gfx950 device visible: the product path never falls back to CPU */
	NRS_ERR_STATE = -5          /* e.g. rendering before params / density grid were set */
} nrs_status;

/* ENerfActivation, include/neural-graphics-primitives/common.h:107 */
typedef enum nrs_activation {
	NRS_ACT_NONE = 0, NRS_ACT_RELU = 1, NRS_ACT_LOGISTIC = 2, NRS_ACT_EXPONENTIAL = 3
} nrs_activation;

/* ERenderMode, common.h:71.  Implemented: AO, Shade, Positions, Depth, Distance, Stepsize, Distortion, Cost, Slice (composite_kernel_nerf's per-sample
 * branches testbed_nerf.cu:905-937, shade_kernel_nerf :2466-2482, init_rays' Distortion branch :2602-2613, the Slice path :3111-3175), and since ABI 3
 * Normals (the network's input gradient, :2924, :905-910, :2466-2468) and EncodingVis (visualized_layer / visualized_dimension, :2926, :925) -- the two
 * modes whose per-sample input lives in tiny-cuda-nn: restated like the forward pass (nrs_network_input_gradient / _visualize_activation below). */
typedef enum nrs_render_mode {
	NRS_RENDER_AO = 0, NRS_RENDER_SHADE = 1, NRS_RENDER_NORMALS = 2, NRS_RENDER_POSITIONS = 3,
	NRS_RENDER_DEPTH = 4, NRS_RENDER_DISTANCE = 5, NRS_RENDER_STEPSIZE = 6, NRS_RENDER_DISTORTION = 7,
	NRS_RENDER_COST = 8, NRS_RENDER_SLICE = 9, NRS_RENDER_ENCODING_VIS = 11 /* ERenderMode::EncodingVis sits behind NumRenderModes (10) */
} nrs_render_mode;

/* GPUMatrixDynamic<T>::layout() of the network output: planes = row-major [16 x n_el]
 * (renderer, density-grid update), interleaved = column-major, 16 halfs per sample (selection, Poisson). */
typedef enum nrs_layout { NRS_PLANES = 0, NRS_INTERLEAVED = 1 } nrs_layout;

/* The two roundings of tiny-cuda-nn that cannot be read off the reference checkout (its tiny-cuda-nn submodule is empty and un-pinned), switchable
 * per model (nrs_model_set_numerics).  Defaults are the wider ones.
 *   grid: FP32    = the trilinear sum of a level runs in fp32 (one fmaf per corner, corners 0..7) and is rounded to fp16 once;
 *         NETWORK = kernel_grid as recalled from NVlabs/tiny-cuda-nn of 2022: per corner `result[f] += (T)(weight * (float)value[f])`, T = __half
 *                   -- the fp32 product is rounded to fp16 and accumulated in fp16.
 *   mlp:  FP32    = fp16 x fp16 products accumulated in fp32 (MFMA accumulators), one rounding per layer output;
 *         FP16    = FullyFusedMLP's wmma fragments carry fp16 accumulators: modelled as one fp16 rounding of the running sum after every 16-wide
 *                   k block (how a tensor core sums inside a block is unspecified: a model of it, within tolerance of any implementation). */
typedef enum nrs_grid_acc { NRS_GRID_ACC_FP32 = 0, NRS_GRID_ACC_NETWORK = 1 } nrs_grid_acc;
typedef enum nrs_mlp_acc { NRS_MLP_ACC_FP32 = 0, NRS_MLP_ACC_FP16 = 1 } nrs_mlp_acc;

/* Network hyper-parameters: configs/nerf/base.json:23-58 + src/testbed.cu:2257-2333.
 * Accepted: base.json's family -- the 16 x 2 hash grid with any table size (base_14 / small / base / big.json: log2_hashmap_size 14 / 15 / 19 / 21), the 64-wide
 * density network with one hidden layer (or none: one [16 x 32] matrix, linear.json), and an rgb network of 0 (CutlassMLP, base_0layer.json), 1, 2 (base.json) or 3 hidden layers (base_{1,2,3}layer.json) on the
 * degree-4 spherical harmonics -- or NO direction encoding and rgb network (base_nodir.json -> NerfNetworkNoDir, testbed.cu:2314-2353): sh_degree = 0,
 * rgb_hidden_layers = 0; the colour is then the density network's outputs 1..3 (nerf_network_nodir.h:47-91).  Parameter blob: [density | rgb | grid] with the rgb part
 * [64 x 32] + (L - 1) [64 x 64] + [16 x 64] for L >= 1 hidden layers, one [8 x 32] matrix for L = 0, nothing for NoDir (tiny-cuda-nn's layouts as recalled;
 * nrs_model_n_params says what a description implies).  Other encodings (configs/nerf/{frequency,densegrid,tensor,...}.json) are refused: NRS_ERR_UNSUPPORTED. */
typedef struct nrs_model_desc {
	uint32_t n_levels;             /* 16 */
	uint32_t n_features_per_level; /* 2  */
	uint32_t log2_hashmap_size;    /* 19 */
	uint32_t base_resolution;      /* 16 */
	float    per_level_scale;      /* exp(ln(2048*aabb_scale/16)/15), testbed.cu:2288-2292 */
	uint32_t n_neurons;            /* 64 (both MLPs) */
	uint32_t density_hidden_layers;/* 1  (0..1) */
	uint32_t density_output_dims;  /* 16, nerf_network_full.h:47-49 */
	uint32_t rgb_hidden_layers;    /* 2  (0..3; 0 with sh_degree 0) */
	uint32_t sh_degree;            /* 4  (0 = NerfNetworkNoDir) */
	uint32_t rgb_activation;       /* nrs_activation; lego: Logistic   (testbed.h:636) */
	uint32_t density_activation;   /* nrs_activation; Exponential      (testbed.h:637) */
	float    aabb_min[3];          /* Testbed::m_aabb (training box): [0,1]^3 for aabb_scale 1 */
	float    aabb_max[3];
} nrs_model_desc;

#define NRS_GRID_SIZE       128u                     /* NERF_GRIDSIZE,  common_nerf.h:16 */
#define NRS_GRID_CASCADES   5u                       /* NERF_CASCADES,  common_nerf.h:26 */
#define NRS_GRID_VOLUME     (128u * 128u * 128u)
#define NRS_BITFIELD_BYTES  (NRS_GRID_VOLUME * NRS_GRID_CASCADES / 8u)   /* 1 310 720 */
#define NRS_NETWORK_INPUT_FLOATS 7u                  /* NerfCoordinate: pos3, dt, dir3; nerf.h:73 */
#define NRS_NETWORK_OUTPUT_WIDTH 16u                 /* padded_output_width() */

/* One cage-deformation operator as the renderer consumes it: the GPU members of TetMesh (tet_mesh.h:80-94)
 * plus the flags CageDeformation::map_rays passes (cage_deformation.cu:547-572).  All arrays are HOST
 * pointers; nrs_edit_create copies them to the device. */
typedef struct nrs_tet_mesh {
	uint32_t        n_vertices;
	uint32_t        n_tets;
	const float*    h_vertices;          /* [V*3] deformed, un-warped world units */
	const float*    h_original_vertices; /* [V*3] canonical */
	const uint32_t* h_tets;              /* [T*4] */
	const uint32_t* h_lut_offsets;       /* [5*128^3 + 1] CSR over level*128^3 + morton, deformed mesh */
	const uint32_t* h_lut_idx;           /* [h_lut_offsets[last]] */
	const uint8_t*  h_original_bitfield; /* [NRS_BITFIELD_BYTES] cells touched by the canonical mesh */
	const float*    h_local_rotations;   /* [T*9] Eigen column-major, or NULL (m_correct_direction off) */
	uint32_t        copy;                /* GrowingSelection::m_copy: keep the source visible */
	/* membrane ("Poisson") correction, cage_deformation.h:163; arrays may be NULL when apply_poisson == 0 */
	uint32_t        apply_poisson;
	float           residual_amplitude;
	const float*    h_boundary_shs;              /* [V*27] SH9RGB per vertex, Eigen col-major 9x3 */
	const float*    h_boundary_outside_density;  /* [V] */
	const float*    h_boundary_residual_density; /* [V] */
	/* Device-side authoring ("next" row f1).  h_lut_offsets == NULL: nrs_edit_create builds the cell->tet LUT of
	 * h_vertices on the device (TetMesh::build_tet_grid, tet_mesh.cu:368); h_original_bitfield == NULL: likewise the
	 * touched cells of h_original_vertices (build_original_tet_grid, :76); h_local_rotations == NULL with
	 * correct_direction != 0: the rotations are computed on the device (update_local_rotations, :37) and kept current
	 * by nrs_edit_update_*.  (m_correct_direction, cage_deformation.h) */
	uint32_t        correct_direction;
} nrs_tet_mesh;

/* AffineDuplication operator (include/.../editing/affine_duplication.h:23-106): the content of an oriented selection box
 * is shown again translated / scaled / rotated.  Fields = what the operator's JSON stores (affine_duplication.cu:356-369);
 * of the selection AffineBoundingBox only center / scale / rot_matrix matter (warp_box and update_destination rebuild
 * u, v, w, min, max from them, affine_bounding_box.cuh:40-101).  Matrices are Eigen column-major 3x3, world units. */
typedef struct nrs_affine_duplication {
	float    selection_center[3];
	float    selection_scale[3];   /* edge lengths of the box */
	float    selection_rot[9];
	float    translation[3];
	float    scale[3];
	float    rotation[9];
	uint32_t hide_original;        /* m_hide_original (false) */
	uint32_t correct_dir;          /* m_correct_dir (true): rotate the view direction too */
} nrs_affine_duplication;

/* Arguments + implicit Testbed members of render_nerf (SURVEY 8b "Renderer"). */
typedef struct nrs_render_params {
	uint32_t struct_size;         /* = sizeof(nrs_render_params) of the header the caller was built with (NRS_RENDER_PARAMS_INIT); anything else is
	                               * NRS_ERR_INVALID_ARG -- the library never reads a struct of another layout */
	int32_t  resolution[2];       /* render_buffer.in_resolution() */
	float    focal_length[2];
	float    camera_matrix0[12];  /* 3x4, Eigen column-major: col0,col1,col2 = axes, col3 = origin */
	float    camera_matrix1[12];
	float    rolling_shutter[4];
	float    screen_center[2];
	float    render_aabb_min[3];  /* m_render_aabb */
	float    render_aabb_max[3];
	uint32_t spp_index;           /* render_buffer.spp(): Sobol sample index */
	uint32_t snap_to_pixel_centers;
	float    min_transmittance;   /* m_nerf.rendering_min_transmittance (0.01) */
	float    cone_angle_constant; /* m_nerf.cone_angle_constant: 0 for aabb_scale 1, 1/256 otherwise */
	uint32_t render_mode;         /* nrs_render_mode (m_render_mode); see the enum for what is implemented */
	uint32_t linear_colors;       /* m_nerf.training.linear_colors: skip srgb_to_linear in shade */
	uint32_t apply_operators;     /* m_enable_edits && !m_distill */
	uint32_t poisson_target;      /* NerfTracer::m_poisson_target */
	uint32_t min_mip;             /* show_accel >= 0 ? show_accel : 0 (marching only) */
	uint32_t max_march_steps;     /* 0 = reference bound (MARCH_ITER, testbed_nerf.cu:56) */
	/* Multi-GPU image-tile sharding (no reference counterpart).  The image is cut into
	 * tile_size x tile_size pixel tiles; tile (Tx, Ty) has the index t = Ty * pitch + Tx with the ODD row pitch
	 * pitch = ceil(W / tile_size) | 1 (nrs_render_tile_pitch) -- with an even pitch and a power-of-two number of ranks, t mod ranks would put
	 * every rank on two columns of tiles; an odd pitch turns the deal into diagonals (max / mean samples per rank at 8 ranks, 32-pixel tiles:
	 * 1.032 -> 1.016).  Indices whose Tx lies beyond the image are virtual (no pixels).  This call renders tiles
	 * t = tile_first, tile_first + tile_stride, ...  tile_size == 0 means "whole image" and frame/depth
	 * are indexed x + W*y.  With tiling, pixel (tx,ty) of the k-th owned tile is written at
	 * ((k * tile_size + ty) * tile_size + tx): a compact buffer ready for one RCCL gather. */
	uint32_t tile_size;           /* multiple of 8, or 0 */
	uint32_t tile_first;
	uint32_t tile_stride;
	/* ---- ABI 2: the remaining implicit Testbed members of render_nerf.  All zero = the behaviour of ABI 1. ---- */
	float    dof;                 /* m_dof: aperture radius of pixel_to_ray's thin-lens branch (common_device.cuh:285-293); 0 = pinhole */
	float    slice_plane_z;       /* m_slice_plane_z + m_scale (testbed_nerf.cu:3067): focus distance of the aperture branch, and the distance
	                               * of the slice plane in render mode Slice (the call negates it itself, :3068-3070) */
	float    depth_scale;         /* 1 / m_nerf.training.dataset.scale (:3113): factor of render modes Depth and Distance */
	uint32_t show_accel;          /* m_nerf.show_accel >= 0 (the level is min_mip): every sample becomes opaque (:788-790) and render mode
	                               * Positions colours the occupancy cell (:911-920) */
	/* camera model and background (init_rays_with_payload_kernel_nerf :2523-2533, 2585-2613; pixel_to_ray common_device.cuh:262-280).  The pointers are
	 * DEVICE pointers for nrs_render_nerf (HOST pointers for the CPU oracle, which takes the same struct); NULL / 0 = absent. */
	uint32_t distortion_mode;     /* ECameraDistortionMode, common.h:166: 0 None, 1 Iterative (OpenCV k1 k2 p1 p2, Newton undistortion :162-199), 2 FTheta (:231-243)
	                               * = m_nerf.render_distortion when m_nerf.render_with_camera_distortion (:3078-3080) */
	float    distortion_params[7];
	const float* d_distortion_map;        /* m_distortion.map->params_inference(): float2 [res.y][res.x], added to the ray's xy (read_image<2>, :278-280) */
	int32_t  distortion_resolution[2];
	int32_t  envmap_resolution[2];
	const float* d_envmap;                /* m_envmap.envmap->params_inference(): float RGBA [res.y][res.x]; every pixel's frame value is REPLACED by the
	                                       * environment seen along its ray before the NeRF composites over it (read_envmap, envmap.cuh:30-63; :2590-2592) */
	uint32_t glow_mode;           /* m_nerf.m_glow_mode: composite_kernel_nerf's grid / cut-line overlay (:806-903); bits 1 green grid, 2 cut line, 4 mask to
	                               * alpha, 8 radial, 16 grid only.  0 = off (the reference's default) */
	float    glow_y_cutoff;       /* m_nerf.m_glow_y_cutoff */
	/* ---- ABI 3: render mode EncodingVis (render_mode = m_visualized_dimension > -1 ? EncodingVis : m_render_mode, testbed_nerf.cu:3072) ---- */
	uint32_t visualized_layer;     /* m_visualized_layer: 0 = hash-grid output (32 wide), 1 = density MLP hidden layer (64), 2 = rgb network input
	                                * (16 density outputs | 16 SH coefficients), 3 / 4 = rgb MLP hidden layers (64); NerfNetworkFull::forward_activations,
	                                * nerf_network_full.h:523-534 */
	uint32_t visualized_dimension; /* m_visualized_dimension (>= 0): the unit of that layer whose activation is shown (< NerfNetworkFull::width(layer), :507-517) */
} nrs_render_params;
/* envmap / distortion map contract: d_envmap holds envmap_resolution[0] x envmap_resolution[1] float4 texels, d_distortion_map
 * distortion_resolution[0] x distortion_resolution[1] float2 texels (both >= 1 x 1, row-major); every lookup clamps (y; the envmap wraps in x) to that extent. */
#define NRS_RENDER_PARAMS_INIT { (uint32_t)sizeof(nrs_render_params) }

typedef struct nrs_render_stats {
	uint64_t n_samples;      /* network-evaluated live samples (sum of per-ray n_steps)            */
	uint32_t n_rays_alive;   /* rays that found an occupied cell (entered the sample loop)          */
	uint32_t n_rays_hit;     /* rays shaded into the frame buffer (alpha > 0.001), = trace()'s n_hit */
} nrs_render_stats;

/* State update_density_grid_nerf_operator reads and advances on Testbed (src/testbed_nerf.cu:3533-3640), handed over
 * explicitly.  One call = one iteration of update_density_grid_nerf_render's loop (:3514-3520), which passes
 * n_uniform = 128^3 * (max_cascade + 1), n_nonuniform = 0 and reset_grid on its first iteration. */
typedef struct nrs_grid_update {
	uint32_t n_uniform_samples;    /* cells drawn with threshold -0.01 (every trained cell)            :3565 */
	uint32_t n_nonuniform_samples; /* cells drawn with threshold NERF_MIN_OPTICAL_THICKNESS (occupied)  :3578 */
	uint32_t reset_grid;           /* zero the float grid first                                         :3558 */
	uint32_t max_cascade;          /* m_nerf.max_cascade: cascades 0..max_cascade are sampled                 */
	float    decay;                /* m_nerf.training.density_grid_decay, 0.95 (testbed.h:604)                */
	uint32_t ema_step;             /* IN/OUT m_nerf.density_grid_ema_step (incremented by the call)     :3636 */
	uint64_t rng_state;            /* IN/OUT m_rng (tcnn::pcg32) state; advanced by 2 * 2^32            :3577,3590 */
	uint64_t rng_inc;              /* m_rng stream constant                                                   */
} nrs_grid_update;

typedef struct nrs_ctx   nrs_ctx;
typedef struct nrs_model nrs_model;
typedef struct nrs_edit  nrs_edit;

const char* nrs_last_error(void);
int         nrs_abi_version(void);

/* ---- context / model ------------------------------------------------------------------------------- */
int  nrs_ctx_create(int device, nrs_ctx** out);
void nrs_ctx_destroy(nrs_ctx* ctx);
int  nrs_ctx_device_info(const nrs_ctx* ctx, char* name_out, size_t name_len, int* n_cus, size_t* hbm_bytes);
/* Lane teams: how many lanes of a wavefront share one ray in nrs_render_nerf.  0 (default) = automatic: 2 or 4 when a
 * launch owns so few pixels (one GPU's tiles of a frame sharded over 4-8 GPUs, small viewports) that its duration would
 * otherwise be one ray's latency chain; one lane per ray for launches that fill the GPU, with teams only for the last
 * third of the frame's work queue ("hybrid", whole-image mode).  1 / 2 / 4 force a size for every ray, -1 forces the
 * hybrid schedule, -2 / -3 / -4 the small-launch schedule (team size chosen per generation from the rays a wave has pending) with packets of 16 / 32 / 64 pixels.
 * Since round 3 the automatic choice is the small-launch schedule with packets sized by the launch; the hybrid schedule runs only when forced.  Pixel values, depth, step counts and statistics do not depend on it (tests/test_gpu_lane_teams.py). */
int  nrs_ctx_set_lane_teams(nrs_ctx* ctx, int lanes_per_ray);
/* Ray hand-over (on by default): in whole-image and small-launch ("hybrid") schedules a wave that has run out of work takes rays from a sibling wave of its
 * workgroup -- rays that wait in the sibling's ring for its next generation, or half of the rays it holds in lanes (both halves then run with more lanes per
 * ray) -- instead of leaving its lanes idle for the frame's tail.  Results do not depend on it (tests/test_gpu_lane_teams.py).  nrs_ctx_ray_handovers reports
 * what the last render launch that returned statistics (h_stats != NULL) handed over: rays moved, hand-overs. */
int  nrs_ctx_set_ray_handover(nrs_ctx* ctx, int enabled);
int  nrs_ctx_ray_handovers(const nrs_ctx* ctx, uint64_t* n_rays, uint64_t* n_handovers);

/* MEMORY NOTE: a model holds its parameters only (24-27 MB).  The cell-record cache -- a memory-for-instructions trade, about 15 % of a lego frame (bench.py key
 * lego_cage_norecords) -- is OPT-IN: nrs_model_set_cell_cache(model, budget) below (10 GiB holds levels 0..11 of base.json's table: 9.2 GB), allocated and filled inside
 * that call and rebuilt inside every later nrs_model_set_params (1.9 ms for 9.2 GB); a caller whose parameters change every frame -- a training viewer -- leaves it off.
 * Results are bit-identical either way.  NRS_CELL_CACHE_GB in the environment switches it on at nrs_model_create for a host that cannot be changed. */
int    nrs_model_create(nrs_ctx* ctx, const nrs_model_desc* desc, nrs_model** out);
void   nrs_model_destroy(nrs_model* model);
/* number of fp16 parameters the description implies (density MLP | rgb MLP | hash grid), host-only */
size_t nrs_model_n_params(const nrs_model_desc* desc);
/* per-level hash-grid table (host-only): scale, resolution, first entry, entry count, hashed flag */
int    nrs_model_level_table(const nrs_model_desc* desc, float* scale, uint32_t* resolution,
                             uint32_t* entry_offset, uint32_t* entry_count, uint32_t* hashed);
/* fp16 parameter blob in tiny-cuda-nn order: density MLP | rgb MLP | hash grid (nerf_network_full.h:316-349).
 * h_params is a HOST pointer (what Trainer::deserialize hands over); synchronous. */
int    nrs_model_set_params(nrs_model* model, const void* h_params_fp16, size_t n_params);
/* The same from a DEVICE pointer, as NerfNetworkFull::set_params receives it (nerf_network_full.h:316-349: pointers into the trainer's blob).
 * Asynchronous: the hash grid is copied device-to-device, the MLP weights are re-arranged into MFMA fragments by a small kernel and the cell
 * records (if any are kept) rebuilt, all enqueued on `stream`; launches enqueued on the same stream afterwards see the new parameters, and the
 * blob may be overwritten once the stream has passed this call.  Copy semantics: call again after every optimiser step. */
int    nrs_model_set_params_device(nrs_model* model, const void* d_params_fp16, size_t n_params, void* stream);
/* nrs_grid_acc / nrs_mlp_acc above.  Applies to every entry point that evaluates the network -- nrs_render_nerf in every schedule, mode and operator
 * combination, the network operators, the occupancy refresh, the grid evaluators, selection rays, the membrane boundary (round 3: no combination is
 * refused any more; the non-default modes run the run-time twins of the kernels, a little slower than the default instantiations). */
int    nrs_model_set_numerics(nrs_model* model, uint32_t grid_acc, uint32_t mlp_acc);
/* Cell-record cache (no counterpart in the reference: a memory-for-bandwidth trade the 288 GB of HBM allow).  For the
 * coarsest levels that fit `max_bytes` (an even number of them), every grid cell gets a 32-byte record holding its 8
 * corner entries, fetched with the level's own index function (tiny-cuda-nn grid.h:76-95), so that a sample reads two
 * 16-byte loads from one cache line instead of hashing eight corners and gathering them from four lines.  Results are
 * bit-identical with or without the cache.  The records are rebuilt inside every nrs_model_set_params (a few ms per
 * 10 GB); callers that change parameters every frame (training) pass 0.  Levels 0..11 of base.json's table take
 * 9.3 GB, 0..13 take 64 GB.  Synchronises the device.  max_bytes = 0 drops the cache. */
int    nrs_model_set_cell_cache(nrs_model* model, size_t max_bytes);
size_t nrs_model_cell_cache_bytes(const nrs_model* model, uint32_t* n_levels_out);
/* Sparse cell records for levels the dense cache cannot hold (aabb_scale-16 scenes: the fine levels of a 16^3-unit box).  The cells of
 * a level are grouped in 8 x 8 x 8 bricks (16 KiB of records); a brick is allocated if it touches a cell marked in h_mask_bitfield (the
 * density-bitfield layout, NRS_BITFIELD_BYTES): pass the occupancy of every place hash-grid lookups can happen -- the current occupancy,
 * OR-ed with the un-edited one when edit operators carry samples back to canonical space.  A sample whose brick has no records gathers the
 * hashed way, so results never depend on the mask, only speed does.  Levels are taken in pairs after the dense ones while brick tables +
 * records fit max_bytes.  Kept current by nrs_model_set_params; dropped by nrs_model_set_cell_cache (set the dense budget first).
 * h_mask_bitfield == NULL or max_bytes == 0 drops them.  Synchronises the device. */
int    nrs_model_set_sparse_cell_cache(nrs_model* model, const uint8_t* h_mask_bitfield, size_t max_bytes);
size_t nrs_model_sparse_cell_cache_bytes(const nrs_model* model, uint32_t* first_level_out, uint32_t* n_levels_out);
/* occupancy: either the ready-made bitfield (NRS_BITFIELD_BYTES, Morton order, mips pooled) ... */
int    nrs_model_set_density_bitfield(nrs_model* model, const uint8_t* h_bitfield, size_t n_bytes);
/* ... or the float density grid [5*128^3]; thresholded with min(0.01, mean) and OR-pooled on the device
 * exactly as update_density_grid_mean_and_bitfield does (testbed_nerf.cu:514-555, 3642-3657). */
int    nrs_model_set_density_grid(nrs_model* model, const float* h_grid, size_t n_floats);
int    nrs_model_get_density_bitfield(nrs_model* model, uint8_t* h_bitfield_out, size_t n_bytes);
/* Test hook: the marching accelerator the library derived from the bitfield (no reference counterpart; the reference marches cell by
 * cell, testbed_nerf.cu:1100-1131).  which 0: the flavour used for general step parameters, 1: for cone_angle == 0 && min_mip == 0.
 * h_box12 = {min[3], max[3], cell[3], 1/cell[3]} of the occupied box and its 32^3 look-ahead blocks, h_mask = 32^3 / 32 words. */
int    nrs_model_get_march_accelerator(nrs_model* model, int which, float* h_box12, uint32_t* h_mask1024);
/* The float grid the bitfield was last derived from ([5*128^3]; zeros if only a bitfield was ever set). */
int    nrs_model_get_density_grid(nrs_model* model, float* h_grid_out, size_t n_floats);
/* Deformed-space occupancy refresh ("next" row f2): Testbed::update_density_grid_nerf_operator, testbed_nerf.cu:3533.
 * Draws grid-cell samples (generate_grid_samples_nerf_nonuniform, common_nerf.cu:179), maps them through the edit
 * operators last-to-first (map_positions, cage_deformation.cu:624), evaluates density(), empties masked samples
 * (clear_empty_space :2759), activates, adds the membrane residual (compute_poisson_residual_density,
 * cage_deformation.cu:645), max-splats per cell (:447), decays (ema_grid_samples_nerf :483) and rebuilds mean,
 * bitfield and mips (:3642) -- all on the device, one fused kernel for everything up to the splat.
 * Synchronous (the reference syncs m_inference_stream at :3519); updates *u. */
int    nrs_model_update_density_grid(nrs_model* model, nrs_edit* const* edits, int n_edits, nrs_grid_update* u, void* stream);
/* tcnn::pcg32(seed) -- Testbed seeds m_rng = default_rng_t{m_seed = 1337} (src/testbed.cu:2220). host-only */
void   nrs_rng_seed(uint64_t seed, uint64_t* state_out, uint64_t* inc_out);

/* ---- multi-GPU: one exchange step per frame (the reference is single-GPU, README.md:423-425) --------------------------- */
/* The frame is cut into tile_size x tile_size tiles dealt round-robin to the ranks (nrs_render_params.tile_*); every rank renders into a compact
 * buffer [tiles_padded * tile^2 * 4 floats of frame | tiles_padded * tile^2 floats of depth]; nrs_gather_tiles moves them to the root with
 * ncclGroupStart / ncclSend / ncclRecv x (N - 1) / ncclGroupEnd (RCCL point-to-point over xGMI) on `stream` and de-tiles there.
 * RCCL is dlopen'ed on first use (no link-time dependency).  Bootstrap as with NCCL: rank 0 makes a 128-byte id, the application distributes
 * it (its own channel), every rank creates the communicator with it (collective call). */
typedef struct nrs_comm nrs_comm;
int  nrs_comm_unique_id(uint8_t* out128);
int  nrs_comm_create(int device, int rank, int n_ranks, const uint8_t* unique_id128, nrs_comm** out);
void nrs_comm_destroy(nrs_comm* comm);
/* What the communicator is: this process's rank, the number of ranks RCCL connected, ncclGetVersion() (0 if the library has none) and the library
 * that was loaded (NRS_RCCL_LIB overrides the search: tests/fake_rccl runs several ranks on one GPU).  Any pointer may be NULL. */
int  nrs_comm_info(const nrs_comm* comm, int* rank_out, int* n_ranks_out, int* rccl_version_out, char* lib_path_out, size_t lib_path_len);
/* Diagnostic (no reference counterpart): `pairs` ncclSend / ncclRecv pairs of n_floats floats from this rank to itself in one group on `stream` -- RCCL's
 * enqueue path of nrs_gather_tiles with one rank, for timing its host-side cost on a one-GPU box (tools/gather_probe.py). d_src / d_dst: pairs * n_floats. */
int  nrs_comm_probe_self_p2p(nrs_comm* comm, const float* d_src, float* d_dst, size_t n_floats, int pairs, void* stream);
/* d_local: this rank's buffer.  Root only: d_recv = n_ranks such buffers (rank-major); d_image [H*W*4] / d_depth [H*W] may be NULL. */
int  nrs_gather_tiles(nrs_ctx* ctx, nrs_comm* comm, int root, const nrs_render_params* p, uint32_t tiles_per_rank_padded, const float* d_local,
                      float* d_recv, float* d_image, float* d_depth, void* stream);

/* ---- NerfNetwork operator -------------------------------------------------------------------------- */
/* d_in: [n x 7] f32 (column-major 7 x n in tcnn terms).  d_out: fp16, n_el = n_padded samples wide:
 * planes -> d_out[c * ld_out + s], interleaved -> d_out[s * 16 + c]; c 0..2 rgb raw, c 3 density raw,
 * c 4..15 the rgb network's padding outputs.  ld_out >= n (planes only). */
int nrs_network_inference(nrs_model* model, void* stream, uint32_t n, const float* d_in,
                          void* d_out_fp16, uint32_t ld_out, int layout);
/* density(): d_in is [n x ld_in] f32 with ld_in 3..7, only floats 0..2 of each record are read
 * (nerf_network_full.h:231-236).  Output = the density MLP's 16 outputs (c 0 = density raw). */
int nrs_network_density(nrs_model* model, void* stream, uint32_t n, const float* d_in, uint32_t ld_in,
                        void* d_out_fp16, uint32_t ld_out, int layout);
/* The network's introspection entry points (tiny-cuda-nn's, restated: the submodule is absent from the reference checkout -- oracle/nrs_oracle.cpp
 * density_input_gradient_one / network_activation_one carry the algorithm and its provenance):
 * nrs_network_input_gradient <- NerfNetwork::input_gradient(stream, 3, positions, gradients) (render mode Normals, src/testbed_nerf.cu:2924; mesh vertex
 *   normals :4491): d density_raw / d position of every sample through the density MLP and the hash grid, backprop scale 128 as in tiny-cuda-nn,
 *   rows 0..2 of the result ([n x 3] f32; rows 3..6 -- dt and the direction -- are zero in the reference's 7-row matrix: the density does not depend on them).
 * nrs_network_visualize_activation <- Network::visualize_activation(stream, layer, dimension, input, output) (render mode EncodingVis, :2926, :3159): unit
 *   `dimension` of NerfNetworkFull::forward_activations(layer) (nerf_network_full.h:523-534: 0 hash grid [32], 1 density hidden [64], 2 rgb network input
 *   = 16 density outputs | 16 SH coefficients, 3 / 4 rgb hidden [64]) as f32 [n]; the reference's output kernel writes max(-v, 0), max(v, 0), 0, 1, 1, 1, 1
 *   into a 7-row matrix -- the caller that wants that picture forms it from v.  d_in is [n x 7] f32. */
int nrs_network_input_gradient(nrs_model* model, void* stream, uint32_t n, const float* d_in, uint32_t ld_in, float* d_grad_out_nx3);
int nrs_network_visualize_activation(nrs_model* model, void* stream, uint32_t layer, uint32_t dimension, uint32_t n, const float* d_in, float* d_out_n);
/* nrs_network_backward <- NerfNetworkFull::backward (nerf_network_full.h:142-221) for base.json's architecture (density_hidden_layers 1, rgb_hidden_layers 2, sh_degree 4,
 *   any log2_hashmap_size, n_extra_dims 0) at the default numerics: the gradient of a loss with respect to every parameter, given dL_doutput.  One persistent launch
 *   that recomputes the forward pass of each 64-sample tile (the values of nrs_network_inference) and stores no activation in global memory.
 *   d_in [n x ld_in] f32, ld_in >= 7.  d_dL_doutput_fp16: planes [16 x ld_dout] (ld_dout >= n) or interleaved [n x 16]; rows 0..2 are the rgb gradients and row 3 the
 *   density's (added onto the density network's output 0 in fp16, add_density_gradient); rows 4..15 are never read (extract_rgb copies three rows).  The gradients pass
 *   the layers in fp16, one rounding per layer boundary, as in tiny-cuda-nn: callers multiply dL_doutput by a loss scale (128 there) and divide the result by it.
 *   d_dL_dparams: nrs_model_n_params floats in the parameter blob's own order, [density | rgb | grid], matrices W[j * n_in + k]; rows 3..15 of the rgb output matrix
 *   come out zero.  fp32 sums (tiny-cuda-nn keeps fp16 gradients: DESIGN.md 4).  accumulate 0: the buffer is zeroed on the stream first (EGradientMode::Overwrite);
 *   1: added to (Accumulate).  Sums are atomic: the last bits depend on the order.
 *   d_dL_dinput: NULL, or [n x ld_in] f32: floats 0..2 of a record receive dL/dposition through the hash grid, floats 3..ld_in-1 are written as zero -- the gradient through the SH
 *   encoding of the direction is not propagated.
 *   NRS_ERR_INVALID_ARG, before any HIP call: a NULL model / d_dL_dparams / (with n > 0) d_in / d_dL_doutput_fp16, ld_in < 7, an unknown layout, planes with ld_dout < n, an n_params
 *   other than the description implies.  NRS_ERR_UNSUPPORTED naming the field: the other networks of the family, light directions, nrs_model_set_numerics other than
 *   FP32 / FP32.  NRS_ERR_STATE before parameters were set.  n = 0 is NRS_OK (the buffer is still zeroed when accumulate is 0).  No allocation, no host
 *   synchronisation.  Callers detect this entry point by symbol (dlsym); NRS_ABI_VERSION is unchanged because no existing layout changes. */
int nrs_network_backward(nrs_model* model, void* stream, uint32_t n, const float* d_in, uint32_t ld_in,
                         const void* d_dL_doutput_fp16, uint32_t ld_dout, int layout, float* d_dL_dparams, size_t n_params, int accumulate,
                         float* d_dL_dinput);
/* The network on a regular grid ("next" row f4: the marching-cubes / volume-export callers of the operator).
 * nrs_density_on_grid <- Testbed::get_density_on_grid (src/testbed_nerf.cu:4538): point (x,y,z) of the res3d grid sits at
 *   aabb_min + (x/rx, y/ry, z/rz) * (aabb_max - aabb_min); d_out[x + y*rx + z*rx*ry] = raw density (fp16 network output as float),
 *   or -10000 where the resident density grid is below NERF_MIN_OPTICAL_THICKNESS at that position (mask_with_density_grid != 0,
 *   grid_samples_half_to_float :464).
 * nrs_rgba_on_grid <- Testbed::get_rgba_on_grid (:4588): the grid spans the render box, every point is seen from ray_dir;
 *   d_out_rgba[i] = (rgb * a, a), a = clamp(1 - exp(-density / 100), 0, 1)  (compute_nerf_density :624). */
int nrs_density_on_grid(nrs_model* model, void* stream, const uint32_t res3d[3], const float aabb_min[3], const float aabb_max[3],
                        int mask_with_density_grid, float* d_out);
int nrs_rgba_on_grid(nrs_model* model, void* stream, const uint32_t res3d[3], const float render_aabb_min[3],
                     const float render_aabb_max[3], const float ray_dir[3], float* d_out_rgba);
/* Selection tool, first step ("next" row f4) <- GrowingSelection::project_selection_pixels (growing_selection.cu:1832-2035:
 * shoot_selection_rays_kernel :1673 + NerfNetwork::density + composite_shot_rays :1768), one launch.  For every scribbled
 * pixel (x, y of `params`' resolution; camera = params->camera_matrix1, focal_length, screen_center, cone_angle_constant)
 * a ray is stepped through the occupied cells of the model's train box (pixel_to_ray with spp 0, direction not
 * normalised, up to NERF_STEPS = 1024 samples) while the density composites; the first sample reached with
 * transmittance <= threshold (the reference's 0.1) gives d_positions[i] (world space) and d_cells[i] =
 * mip * 128^3 + morton(cell); d_found[i] = 0 and position = aabb_min - 1 when the ray never gets there.  The camera is a PINHOLE whatever the lens fields
 * of `params` say: the reference's shoot_selection_rays_kernel calls pixel_to_ray with its default arguments (growing_selection.cu:1696-1703: no distortion,
 * no aperture, spp 0), so dof / distortion_* / d_distortion_map are not read here -- unlike nrs_render_nerf and nrs_trace_samples, which march the lens
 * the renderer uses. */
int nrs_project_selection_pixels(nrs_model* model, void* stream, const nrs_render_params* params, const int32_t* d_pixels_xy,
                                 uint32_t n_pixels, float transmittance_threshold, float* d_positions, uint32_t* d_cells, uint8_t* d_found);
/* host-only bookkeeping that follows (:1964-2021): automatic growing level = highest cascade found, cells below it lifted
 * to it (get_upper_cell_idx, selection_utils.cu:36), duplicates dropped; outputs in pixel order, sized n. */
uint32_t nrs_upper_cell_idx(uint32_t cell_idx, uint32_t target_level);
int nrs_selection_cells(const float* h_positions, const uint32_t* h_cells, const uint8_t* h_found, uint32_t n, int automatic_max_level,
                        uint32_t* growing_level_inout, uint32_t* out_cells, float* out_positions, uint32_t* n_out);
/* Membrane ("Poisson") boundary values of a proxy cage ("next" row f4) <- GrowingSelection::compute_poisson_boundary
 * (growing_selection.cu:2220-2348): for every cage vertex, sh_width^2 directions on the sphere (stratified in (u, v) with one
 * jitter pair per sample -- the reference draws them with std::rand(); here the caller supplies them, [n_verts * sh_width^2][2]
 * in [0, 1]), the full network at the vertex seen from those directions, then the vertex's density (its first sample; zeroed
 * where the occupancy is empty when is_inside, filter_empty :2200) and the SH9 fit of the colours (project_sh9, times
 * 4 pi / n).  h_sh_out: [n_verts][27], SH9RGB column-major (coefficient k of colour c at 9 c + k) -- what the render path's
 * membrane correction consumes.  Host pointers, synchronous, like the reference.  nrs_poisson_sample_coords is the host half
 * on its own (the [n][7] network inputs), exported for tests. */
int  nrs_poisson_boundary(nrs_model* model, const float* h_vertices, uint32_t n_verts, uint32_t sh_width, uint32_t hemisphere_width,
                          const float* h_jitter, int is_inside, float* h_density_out, float* h_sh_out);
void nrs_poisson_sample_coords(const float* vertices, uint32_t n_verts, uint32_t sh_width, uint32_t hemisphere_width, const float* jitter,
                               const float aabb_min[3], const float aabb_max[3], float* coords7_out);
/* hash-grid encoding alone (test hook; tcnn Encoding::inference_mixed_precision): d_out [n x 32] fp16 */
int nrs_hashgrid_encode(nrs_model* model, void* stream, uint32_t n, const float* d_in, uint32_t ld_in,
                        void* d_out_fp16);

/* ---- edit operators -------------------------------------------------------------------------------- */
int  nrs_edit_create(nrs_ctx* ctx, const nrs_model_desc* desc, const nrs_tet_mesh* mesh, nrs_edit** out);
/* AffineDuplication(selection_box, translation, aabb) + update_destination (affine_duplication.h:26, 77-90); the
 * resulting nrs_edit is used exactly like a cage edit (map_rays / map_positions / render / occupancy refresh). */
int  nrs_edit_create_affine(nrs_ctx* ctx, const nrs_model_desc* desc, const nrs_affine_duplication* op, nrs_edit** out);
void nrs_edit_destroy(nrs_edit* edit);
/* map_rays: in-place on d_coords [n x 7] f32, OR-accumulates into d_empty_mask [n] u8 */
int  nrs_edit_map_rays(nrs_edit* edit, void* stream, uint32_t n, float* d_coords, uint8_t* d_empty_mask);
/* map_positions: in-place on d_pos [n x ld] f32 (ld >= 3), OR-accumulates into d_empty_mask */
int  nrs_edit_map_positions(nrs_edit* edit, void* stream, uint32_t n, float* d_pos, uint32_t ld,
                            uint8_t* d_empty_mask);

/* Per-gizmo-move chain on the device ("next" row f1).  The reference redoes all of this on the CPU for every move and
 * re-uploads ~45 MB (tet_mesh.cu:651-667); here only the cage vertices (or the tet vertices) cross PCIe.
 *   nrs_edit_set_mvc          <- Cage::compute_mvc's result (cage.cu:6), [V x n_cage_vertices] row-major, uploaded once
 *   nrs_edit_update_cage      <- Cage::interpolate_with_mvc (cage.cu:38) + TetMesh::post_update_vertices (tet_mesh.cu:12)
 *                                + build_tet_grid (:368) + update_local_rotations (:37)
 *   nrs_edit_update_vertices  <- the same chain from explicit deformed tet vertices (TetMesh::update_vertices)
 * Both synchronise `stream` (the LUT size and the bounding box come back to the host), like the reference's host code. */
int  nrs_edit_set_mvc(nrs_edit* edit, const float* h_weights, uint32_t n_cage_vertices);
int  nrs_edit_update_cage(nrs_edit* edit, void* stream, const float* h_cage_vertices, uint32_t n_cage_vertices);
int  nrs_edit_update_vertices(nrs_edit* edit, void* stream, const float* h_vertices, uint32_t n_vertices);
int  nrs_edit_lut_size(const nrs_edit* edit, uint32_t* n_idx_out, uint32_t* max_per_cell_out);
/* GrowingSelection::interpolate_poisson_boundary (src/editing/tools/growing_selection.cu:2350-2395): the link between nrs_poisson_boundary
 * (membrane terms per CAGE vertex, inside and outside) and the renderer's membrane path (terms per TET vertex): boundary_shs, outside density and
 * residual density of every tet vertex as gamma-weighted sums over the cage vertices.  h_gamma = TetMesh::gamma_coordinates [V x n_cage_vertices]
 * (= compute_mvc of the canonical vertices with mvc_gamma); NULL: the weights given to nrs_edit_set_mvc (mvc_gamma = 1, the default).
 * The operator then applies the membrane correction (apply_poisson, residual_amplitude) in every later render.  Synchronises `stream`. */
int  nrs_edit_poisson_interpolate(nrs_edit* edit, void* stream, const float* h_gamma, uint32_t n_cage_vertices, const float* h_inside_density,
                                  const float* h_outside_density, const float* h_inside_shs, const float* h_outside_shs, float residual_amplitude);
int  nrs_edit_download_poisson(nrs_edit* edit, float* h_boundary_shs, float* h_outside_density, float* h_residual_density);
/* read the device-side tables back (tests / inspection); any pointer may be NULL.  h_lut_idx holds n_idx entries,
 * h_bbox6 = min xyz, max xyz of the deformed mesh. */
int  nrs_edit_download(nrs_edit* edit, float* h_vertices, uint32_t* h_lut_offsets, uint32_t* h_lut_idx, float* h_rotations,
                       uint8_t* h_original_bitfield, float* h_bbox6);

/* ---- renderer -------------------------------------------------------------------------------------- */
/* d_frame: f32x4 premultiplied linear RGBA, pre-cleared by the caller (clear_frame, testbed.cu:2635);
 * d_depth: f32 (written 1e10 for every pixel of the owned tiles first, as init_rays does);
 * d_steps: optional u32 per pixel = samples composited (the reference's payload.n_steps, tn:957-960, minus the one it counts for a ray that ran out of samples), may be NULL.
 * edits are applied last-to-first (testbed_nerf.cu:2899).  h_stats may be NULL; when non-NULL the call
 * synchronises the stream before returning (the reference's trace() syncs to read n_hit). */
int nrs_render_nerf(nrs_model* model, const nrs_render_params* params, nrs_edit* const* edits, int n_edits,
                    float* d_frame, float* d_depth, uint32_t* d_steps, void* stream, nrs_render_stats* h_stats);
/* spp accumulation <- CudaRenderBuffer::accumulate (src/render_buffer.cu:540-560; accumulate_kernel :217-254): d_accumulate [H*W] f32x4 becomes the running mean
 * of the frames rendered so far for this view; sample_count = frames already in it (0: the buffer is overwritten, as the reference clears it first).  The caller
 * renders frame k with spp_index = k (the Sobol pixel offsets, snap_to_pixel_centers off) into a cleared d_frame and calls this: scripts/run.py's 8-spp test
 * images are 8 such rounds.  color_space = EColorSpace (common.h:122): Linear | SRGB (linear_to_srgb applied to the frame before the mean) | VisPosNeg (EncodingVis). */
typedef enum nrs_color_space { NRS_COLOR_LINEAR = 0, NRS_COLOR_SRGB = 1, NRS_COLOR_VISPOSNEG = 2 } nrs_color_space;
int nrs_accumulate(nrs_ctx* ctx, void* stream, uint32_t width, uint32_t height, const float* d_frame, float* d_accumulate, uint32_t sample_count, uint32_t color_space);
/* number of tiles this rank owns / pixels of the compact buffer for given params (host-only; virtual tiles of the odd pitch included) */
uint32_t nrs_render_owned_tiles(const nrs_render_params* params);
/* the row pitch of the tile index: ceil(W / tile_size) | 1 (0 when tile_size == 0) */
uint32_t nrs_render_tile_pitch(const nrs_render_params* params);
/* scatter compact tile buffers of all ranks (rank-major, as a gather delivers them) back into a full W x H image.
 * Rank r's tiles start at d_tiles + r * rank_stride_floats (0 = densely packed: tiles_per_rank_padded * tile^2 * channels);
 * a stride lets frame and depth share one gathered buffer [rank][frame block | depth block] -> one collective per frame. */
int nrs_detile(nrs_ctx* ctx, void* stream, const nrs_render_params* params, uint32_t n_ranks,
               uint32_t tiles_per_rank_padded, const float* d_tiles, uint32_t channels, size_t rank_stride_floats, float* d_image);
/* Test hook for bit-exact ray/sample indexing: for each listed pixel, march exactly as the renderer does
 * (init -> jitter -> first hit -> successive samples) ignoring compositing, and emit up to max_samples
 * (t, dt) pairs.  d_t, d_dt: [n_pixels x max_samples] f32; d_count: [n_pixels] u32. */
int nrs_trace_samples(nrs_model* model, const nrs_render_params* params, void* stream, uint32_t n_pixels,
                      const uint32_t* d_pixel_idx, uint32_t max_samples, float* d_t, float* d_dt, uint32_t* d_count);

/* ---- on-disk formats either side of the path ("next" row f3; host-only, no device needed) ------------------------ */
/* Snapshot: Testbed::load_network_config + load_snapshot (src/testbed.cu:152-184, 3054-3087).  `.msgpack` is
 * nlohmann::json::to_msgpack of the network config with a "snapshot" object; `.ingp` is the same behind zlib (zstr).
 * Read here: encoding / network / rgb_network / dir_encoding hyper-parameters, snapshot.nerf.aabb_scale (or
 * .dataset.aabb_scale), snapshot.params_binary (tcnn Trainer::serialize, fp16 or float), snapshot.density_grid_binary
 * (float [5*128^3] from save_snapshot, fp16 [(max_cascade+1)*128^3] from export_snapshot), snapshot.camera.matrix. */
typedef struct nrs_snapshot nrs_snapshot;
/* (a snapshot trained with light directions is refused here: nrs_snapshot_open_ex with NRS_SNAPSHOT_ALLOW_LIGHT_DIRS, at the end of this header, reads it) */
int          nrs_snapshot_open(const char* path, nrs_snapshot** out);
void         nrs_snapshot_close(nrs_snapshot* snapshot);
int          nrs_snapshot_model_desc(const nrs_snapshot* snapshot, nrs_model_desc* desc_out, uint32_t* aabb_scale_out);
const void*  nrs_snapshot_params_fp16(const nrs_snapshot* snapshot, size_t* n_params_out);   /* -> nrs_model_set_params */
const float* nrs_snapshot_density_grid(const nrs_snapshot* snapshot, size_t* n_floats_out);  /* -> nrs_model_set_density_grid */
int          nrs_snapshot_camera(const nrs_snapshot* snapshot, float* camera_matrix12_out);   /* column-major 3x4 */
/* Edits: Testbed::load_edits (src/testbed.cu:3205-3236): {"edit_operators": [{"type": "cage_deformation",
 * "proxy_cage": Cage (cage.h:100-145), "interpolation_mesh": TetMesh (tet_mesh.h:136-174), ...}]}.
 * nrs_edits_cage fills an nrs_tet_mesh for DEVICE authoring (vertices, original vertices, tets; LUT / bitfield /
 * rotations left NULL so nrs_edit_create builds them, as the reference's JSON constructor rebuilds the tet grid,
 * growing_selection.cu:112-115) and hands out the MVC weights and the proxy cage.  Pointers live as long as `edits`.
 * An operator saved before its cage was tetrahedralised has no interpolation mesh (growing_selection.cu:2477): mesh_out->n_tets == 0, the cage is still returned.
 * Empty lists may appear as `null` in the file (the reference's vector writers leave an empty vector's value untouched, json_binding.h:231-321): read as empty. */
typedef struct nrs_edits nrs_edits;
int          nrs_edits_open(const char* path, nrs_edits** out);
void         nrs_edits_close(nrs_edits* edits);
uint32_t     nrs_edits_count(const nrs_edits* edits);
const char*  nrs_edits_type(const nrs_edits* edits, uint32_t i);   /* "cage_deformation", "affine_duplication", "twist" */
int          nrs_edits_affine(const nrs_edits* edits, uint32_t i, nrs_affine_duplication* op_out);
int          nrs_edits_cage(const nrs_edits* edits, uint32_t i, nrs_tet_mesh* mesh_out, const float** h_mvc_weights_out,
                            const float** h_cage_vertices_out, const float** h_cage_original_vertices_out,
                            const uint32_t** h_cage_triangles_out, uint32_t* n_cage_vertices_out, uint32_t* n_cage_triangles_out);

/* ---- host-side edit authoring ("next" row f1; CPU like the reference, no device needed) -------------- */
typedef struct nrs_tet_lut nrs_tet_lut;
/* builds the cell->tet CSR of `h_vertices` and the touched-cell bitfield; n_threads 0 = hardware */
int  nrs_tet_lut_build(const float* h_vertices, uint32_t n_vertices, const uint32_t* h_tets, uint32_t n_tets,
                       int n_threads, nrs_tet_lut** out);
uint32_t        nrs_tet_lut_n_idx(const nrs_tet_lut* lut);
uint32_t        nrs_tet_lut_max_per_cell(const nrs_tet_lut* lut);
const uint32_t* nrs_tet_lut_offsets(const nrs_tet_lut* lut);   /* [5*128^3+1] */
const uint32_t* nrs_tet_lut_idx(const nrs_tet_lut* lut);
const uint8_t*  nrs_tet_lut_bitfield(const nrs_tet_lut* lut);  /* [NRS_BITFIELD_BYTES] */
void            nrs_tet_lut_destroy(nrs_tet_lut* lut);
/* MVC weights of n_points points w.r.t. a closed triangulated cage (mvc.h:125-188), float arithmetic.
 * h_weights_out [n_points x n_cage_vertices]; h_labels_out [n_points] (1 = degenerate case hit), may be NULL */
int nrs_mvc_compute(const float* h_cage_vertices, uint32_t n_cage_vertices, const uint32_t* h_cage_triangles,
                    uint32_t n_cage_triangles, const float* h_points, uint32_t n_points,
                    float* h_weights_out, uint8_t* h_labels_out);
/* points[i] = sum_j w[i][j] * cage[j]   (cage.cu:38-49) */
int nrs_mvc_apply(const float* h_weights, const float* h_cage_vertices, uint32_t n_cage_vertices,
                  uint32_t n_points, float* h_points_out);
/* per-tet deformed->canonical rotation R = U V^T of sum (orig-c0)(def-c1)^T (tet_mesh.cu:37-74); [T*9] col-major */
int nrs_tet_local_rotations(const float* h_vertices, const float* h_original_vertices, const uint32_t* h_tets,
                            uint32_t n_tets, float* h_rotations_out);

/* ---- several samples per pixel of one view in one launch ------------------------------------------------------------ */
/* What an offline caller of the reference does with a still view -- render_to_cpu (src/python_api.cu:129) and scripts/run.py --screenshot_spp / --video_spp loop
 * `spp` times over render + accumulate -- as ONE launch of the render kernel and ONE pass over the accumulate buffer.  Callers detect the two entry points by symbol
 * (dlsym); NRS_ABI_VERSION is unchanged because no existing layout changes.
 *
 * nrs_render_nerf_spp renders samples params->spp_index + k, k = 0 .. spp_count - 1, of the view `params` describes: the packet queue of the persistent kernel holds the
 * packets of all spp_count samples (one dispatch ramp, one staging of the weights, one drain).  Sample k is written to slab k of each buffer: what nrs_render_nerf
 * writes at pixel index i of d_frame / d_depth / d_steps lands at k * slab_stride_pixels + i of d_frames (f32x4) / d_depths (f32) / d_steps (u32, may be NULL).  Every
 * frame slab is pre-cleared by the caller exactly as d_frame is for nrs_render_nerf.  Each slab is bit-equal to the output of nrs_render_nerf with spp_index + k, and
 * h_stats is the sum over the samples.  spp_count == 1 is nrs_render_nerf.
 * NRS_ERR_INVALID_ARG, with the argument named in the message:
 *   spp_count == 0 or > NRS_SPP_BATCH_MAX;
 *   slab_stride_pixels smaller than the pixels one call owns (W * H, or owned tiles * tile_size^2 in tiled mode), or spp_count * slab_stride_pixels >= 2^32;
 *   spp_count > 1 and a resolution above NRS_SPP_BATCH_MAX_RESOLUTION in either axis (a pending ray's record holds the sample beside the pixel);
 *   spp_count times the packets, or the pixels, of one sample beyond 2^30 (the 32-bit packet counter);
 *   render mode Slice with spp_count > 1: a slice has no per-sample jitter beyond the pixel offset and no persistent launch to share -- loop over the single-frame call;
 *   and everything the single-frame call refuses (the checks are the same code).
 * The schedule is chosen from the rays of the whole batch.  A batch launch leaves the hit-share feedback that sizes the caller's next single-frame launch untouched. */
#define NRS_SPP_BATCH_MAX 64u
#define NRS_SPP_BATCH_MAX_RESOLUTION 8192
int nrs_render_nerf_spp(nrs_model* model, const nrs_render_params* params, nrs_edit* const* edits, int n_edits, uint32_t spp_count,
                        float* d_frames, float* d_depths, uint32_t* d_steps, size_t slab_stride_pixels, void* stream, nrs_render_stats* h_stats);
/* Folds the spp_count slabs into the running mean in sample order: bit-equal to spp_count calls of the single-frame accumulate with sample_count, sample_count + 1, ...
 * (the per-sample update of accumulate_kernel inside a loop over the slabs: the running mean is not associative), with one read and one write of d_accumulate. */
int nrs_accumulate_spp(nrs_ctx* ctx, void* stream, uint32_t width, uint32_t height, const float* d_frames, size_t slab_stride_pixels, uint32_t spp_count,
                       float* d_accumulate, uint32_t sample_count, uint32_t color_space);
/* Introspection: render-kernel dispatches this context has enqueued so far (a batch of any size is one), and the schedule of the last one:
 * lanes per ray (0 = sized per generation) | lanes on a pixel during the fill << 8 | small-launch schedule << 16 | hybrid queue << 17 | BATCH twin << 18 |
 * a view per sample (nrs_render_nerf_spp_views) << 19.  Either may be NULL. */
int nrs_ctx_render_launches(const nrs_ctx* ctx, uint64_t* n_dispatches_out, uint32_t* last_schedule_out);

/* ---- a view per sample: motion-blurred frames of a moving camera in one launch ------------------------------------------------------------ */
/* Testbed::render_to_cpu (src/python_api.cu:129-175) renders each of the `spp` samples of a frame with its own pair of cameras -- log_space_lerp of the frame's start and
 * end camera at the sample's share of the shutter -- and, over a camera path, with its own fov, aperture and focus plane (set_camera_from_time per sample): the video loop
 * of scripts/run.py.  Callers detect these entry points by symbol (dlsym); NRS_ABI_VERSION is unchanged because no existing layout changes.
 *
 * nrs_render_nerf_spp_views is nrs_render_nerf_spp with a view per sample: sample k renders as nrs_render_nerf does with `params` whose camera_matrix0 / camera_matrix1 /
 * focal_length / dof / slice_plane_z are h_views[k]'s and whose spp_index is spp_index + k; slab k (frame, depth, steps) is bit-equal to that call's output and h_stats is
 * the sum over the samples.  The six fields of `params` itself are not read.  h_views is a HOST array of spp_count records, copied inside the call (the caller may free it
 * on return); the copy is ordered on `stream` and adds no synchronisation.  h_views == NULL is nrs_render_nerf_spp; spp_count == 1 is one nrs_render_nerf of that view.
 * Refused like nrs_render_nerf_spp (the same code, the per-view fields checked for every view), and NRS_ERR_INVALID_ARG naming h_views[k].<field> for a non-finite value
 * or a focal_length <= 0 in any view. */
typedef struct nrs_sample_view {          /* what render_frame() receives per sample inside render_to_cpu's loop */
	float camera_matrix0[12], camera_matrix1[12]; /* as in nrs_render_params */
	float focal_length[2];
	float dof;
	float slice_plane_z;                  /* already m_slice_plane_z + m_scale, as in nrs_render_params */
} nrs_sample_view;
int nrs_render_nerf_spp_views(nrs_model* model, const nrs_render_params* params, nrs_edit* const* edits, int n_edits, uint32_t spp_count, const nrs_sample_view* h_views,
                              float* d_frames, float* d_depths, uint32_t* d_steps, size_t slab_stride_pixels, void* stream, nrs_render_stats* h_stats);

/* The cameras of render_to_cpu's loop: host-only functions (no GPU, no context).  The camera math is evaluated in double and rounded once to float: a restatement of the
 * reference's formulas, not of Eigen's float evaluation of the matrix functions.  Camera matrices are 3x4 column-major [12], as everywhere in this header.
 *
 * nrs_log_space_lerp <- log_space_lerp (src/common_device.cu:27-36): exp(t * log(B * A^-1)) * A on the 4x4 completions of begin (A) and end (B).  begin == end returns it
 *   exactly.  NRS_ERR_INVALID_ARG for a non-finite entry or a singular `begin`; NRS_ERR_UNSUPPORTED where B * A^-1 has no real logarithm the series can reach
 *   (an eigenvalue on the negative real axis: a rotation by exactly 180 degrees).
 * nrs_camera_keyframe <- CameraKeyframe (include/neural-graphics-primitives/camera_path.h:30-36); R is the quaternion (x, y, z, w).
 * nrs_camera_keyframe_matrix <- CameraKeyframe::m() (:37-42): the normalised quaternion's rotation matrix beside T.
 * nrs_camera_keyframe_from_matrix <- the constructor of :53 (Eigen's matrix -> quaternion conversion); slice / scale / fov / dof are copied from the arguments.
 * nrs_camera_path_eval <- CameraPath::eval_camera_path (:74-81) and spline (src/camera_path.cu:50-68): the cubic B-spline over the four keyframes around t * (n - 1),
 *   indices clamped, weights in float, p0 * a + p1 * b + p2 * c + p3 * d summed left to right with operator+'s sign flip of the right-hand quaternion (:55-59).
 *   n == 0 returns the zero keyframe (a default-constructed one in the reference).
 * nrs_camera_path_open / _count / _keyframes / _close <- CameraPath::load (src/camera_path.cu:114-136; load_relative_to_first = false): the
 *   {"time", "path": [{"R", "T", "slice", "scale", "fov", "dof"}]} file CameraPath::save writes.  A missing "path" or an empty one gives zero keyframes; a keyframe without
 *   one of its six keys is NRS_ERR_INVALID_ARG naming the key, as every unreadable file is.
 * nrs_motion_views <- lines 148-158 of src/python_api.cu for samples i = first_sample .. first_sample + spp_count - 1 of spp_total: out_views[k].camera_matrix0 / 1 =
 *   log_space_lerp(start, end, i / spp_total * shutter_fraction) / (..., (i + 1) / spp_total * shutter_fraction).  With n_keys > 0 and start_time >= 0 the keyframe at
 *   start_time + (end_time - start_time) * (alpha0 + alpha1) / 2 gives focal_length (both axes fov_to_focal_length(1, fov) * resolution[fov_axis],
 *   common_device.cuh:444-446 and Testbed::calc_focal_length with zoom 1), dof and slice_plane_z = slice + scale; otherwise they are base_view's. */
typedef struct nrs_camera_keyframe { float R[4], T[3], slice, scale, fov, dof; } nrs_camera_keyframe;
typedef struct nrs_camera_path nrs_camera_path;
int nrs_log_space_lerp(const float begin[12], const float end[12], float t, float out[12]);
int nrs_camera_keyframe_matrix(const nrs_camera_keyframe* key, float out[12]);
int nrs_camera_keyframe_from_matrix(const float matrix[12], float slice, float scale, float fov, float dof, nrs_camera_keyframe* out);
int nrs_camera_path_eval(const nrs_camera_keyframe* keys, uint32_t n_keys, float t, nrs_camera_keyframe* out);
int nrs_camera_path_open(const char* path, nrs_camera_path** out);
uint32_t nrs_camera_path_count(const nrs_camera_path* path);
int nrs_camera_path_keyframes(const nrs_camera_path* path, nrs_camera_keyframe* out, uint32_t capacity);
void nrs_camera_path_close(nrs_camera_path* path);
int nrs_motion_views(const float start[12], const float end[12], float shutter_fraction, uint32_t spp_count, uint32_t first_sample, uint32_t spp_total,
                     const int32_t resolution[2], int fov_axis, const nrs_camera_keyframe* keys, uint32_t n_keys, float start_time, float end_time,
                     const nrs_sample_view* base_view, nrs_sample_view* out_views);

/* ---- networks trained with light directions (n_extra_dims = 3) ----------------------------------------------------------------------- */
/* dataset.has_light_dirs sets n_extra_dims = 3 (src/testbed.cu:2318): NerfNetworkFull builds the direction encoding over n_dir_dims + n_extra_dims inputs
 * (nerf_network_full.h:43), every sample carries three more floats behind its NerfCoordinate (nerf.h:73-96, set_with_optional_light_dir), and rendering passes ONE light
 * direction per frame, m_nerf.light_dir.normalized() (testbed.h:639, src/testbed_nerf.cu:3135, :649, :690), as do the selection and Poisson callers
 * (growing_selection.cu:1914, :2230).  Callers detect these entry points by symbol (dlsym); NRS_ABI_VERSION is unchanged because no existing layout changes.
 *
 * The network (tiny-cuda-nn as recalled; unpinned like the rest of that boundary): the direction encoding is configs/nerf/base.json:37-51's Composite
 * [SphericalHarmonics(3 dims, degree 4) | Identity(the remaining 3 dims)] = 19 outputs, padded to 32.  The rgb network's input is 48 wide: columns 0..15 the density network's
 * outputs, 16..31 the SH coefficients, 32..34 warp_direction(l) = (l + 1) / 2 in fp32 rounded to fp16, 35..47 padding that the Identity kernel writes as 1 -- those weight
 * columns act as a learned bias.  The first rgb matrix is [64 x 48] row-major, the blob 64 * 16 halfs longer; nothing else of the network changes.
 * Supported: sh_degree = 4 with rgb_hidden_layers 1..3.  NerfNetworkNoDir and the 0-layer CutlassMLP rgb network with extra dims: NRS_ERR_UNSUPPORTED.
 *
 * nrs_model_create_ex: n_extra_dims 0 (= nrs_model_create) or 3; anything else is NRS_ERR_UNSUPPORTED.  nrs_model_set_params / _device then take the longer blob.
 * nrs_model_n_params_ex: the plain count + 1024 for n_extra_dims = 3 (0 for what nrs_model_create_ex refuses).
 * nrs_model_set_light_dir <- m_nerf.light_dir: normalised at use, default (0.5, 0.5, 0.5); a zero (or non-finite) vector is NRS_ERR_INVALID_ARG; on a model without extra dims the
 *   call is accepted and has no effect.  The current light direction is what EVERY entry point feeds to every sample when the caller gives no per-sample values:
 *   nrs_render_nerf / _spp (Slice included), nrs_network_inference (7-float records), nrs_rgba_on_grid, nrs_poisson_boundary, nrs_network_visualize_activation and render mode
 *   EncodingVis (layer 2 is 48 wide: units 32..34 the warped light, 35..47 are 1).  Density-only entry points are unaffected.  Edit operators rotate the view direction only
 *   (cage_deformation.cu:547-572 touches floats 4..6).
 * nrs_render_nerf with such a model: every combination is served except the membrane correction (an edit with apply_poisson while apply_operators is set) and the
 *   measurement routes (NRS_DEV_KNOBS: the wave log, NRS_RENDER_CFG), which return NRS_ERR_UNSUPPORTED -- such a model is never rendered without its light term.
 * nrs_network_inference_strided <- inference with PitchedPtr<NerfCoordinate> + extra_stride: records of ld_in >= 7 floats; with ld_in >= 10 on a model with extra dims, floats
 *   7..9 of a record are that sample's ALREADY-WARPED light direction; with ld_in 7..9 the model's light direction is used; on a model without extra dims floats beyond 6 are ignored. */
int    nrs_model_create_ex(nrs_ctx* ctx, const nrs_model_desc* desc, uint32_t n_extra_dims, nrs_model** out);
size_t nrs_model_n_params_ex(const nrs_model_desc* desc, uint32_t n_extra_dims);
int    nrs_model_n_extra_dims(const nrs_model* model);
int    nrs_model_set_light_dir(nrs_model* model, const float dir[3]);
int    nrs_network_inference_strided(nrs_model* model, void* stream, uint32_t n, const float* d_in, uint32_t ld_in, void* d_out_fp16, uint32_t ld_out, int layout);
/* nrs_snapshot_open with flags.  NRS_SNAPSHOT_ALLOW_LIGHT_DIRS: a snapshot trained with light directions -- recognised by the keys a writer may add (has_light_dirs /
 * n_extra_dims) and by the size of its parameter blob, exactly as nrs_snapshot_open recognises (and refuses) it -- is read: nrs_snapshot_n_extra_dims answers 3 and
 * nrs_snapshot_params_fp16 hands out the longer blob for nrs_model_create_ex(..., 3, ...).  flags = 0 is nrs_snapshot_open. */
#define NRS_SNAPSHOT_ALLOW_LIGHT_DIRS 1u
int      nrs_snapshot_open_ex(const char* path, uint32_t flags, nrs_snapshot** out);
uint32_t nrs_snapshot_n_extra_dims(const nrs_snapshot* snapshot);

/* ---- tonemap: the display step after accumulate, with 8-bit output ------------------------------------------------------------------------- */
/* Testbed::render_frame ends in render_buffer.accumulate(...) and render_buffer.tonemap(m_exposure, m_background_color, to_srgb ? SRGB : Linear, stream)
 * (src/testbed.cu:2761-2762); render_to_cpu hands back the tonemapped surface (src/python_api.cu:129-175).  Callers detect these entry points by symbol (dlsym);
 * NRS_ABI_VERSION is unchanged because no existing layout changes.
 *
 * nrs_tonemap <- CudaRenderBuffer::tonemap (src/render_buffer.cu:562-580; tonemap_kernel :471-501, tonemap and its curves :254-332, linear_to_srgb / srgb_to_linear
 * common_device.cuh:31-61, EColorSpace / ETonemapCurve common.h:122-135).  Per pixel of d_accumulate [H*W] f32x4, in the reference's operation order:
 *   background: rgb of background_color through srgb_to_linear unless color_space is SRGB; weight = (1 - a) * bg.a; rgb += bg.rgb * weight; a += weight;
 *   srgb_to_linear if color_space is SRGB;  rgb *= 2^exposure;  the curve (Identity returns x untouched, the others start from max(x, 0));
 *   linear_to_srgb if output_color_space is SRGB;  all four channels clamped to [0, 1] if clamp_output.
 * Plain fp32 (bit-reproducible) except the powf of the two sRGB curves.  d_out [H*W]:
 *   NRS_TONEMAP_RGBA32F  f32x4 per pixel, the reference's surface / lopi content.  d_out may be d_accumulate itself (in place).
 *   NRS_TONEMAP_RGBA8    one packed dword per pixel, bytes R, G, B, A in memory, each (uint32_t)(min(max(c, 0), 1) * 255 + 0.5f): the clamp is implied.  Must not alias d_accumulate.
 * nrs_tonemap_output_bytes: the size of d_out (16 or 4 bytes per pixel; 0 for an unknown format).
 *
 * nrs_accumulate_spp_tonemap: nrs_accumulate_spp (color_space taken from the params) followed by nrs_tonemap of the result, in one pass: the K slabs are read, d_accumulate
 * is read once and written once, d_out is written once.  d_accumulate and d_out are bit-equal to what the two calls leave.  d_out must alias neither d_frames nor d_accumulate.
 *
 * NRS_ERR_INVALID_ARG before any device is touched, with the argument named in the message: a NULL ctx, buffer or params; struct_size smaller than the struct;
 * width or height 0; color_space > 2; output_color_space > 1; tonemap_curve > 3; clamp_output > 1; an unknown output_format; a non-finite exposure; and, for the fused
 * call, everything nrs_accumulate_spp refuses. */
typedef enum nrs_tonemap_curve { NRS_TONEMAP_IDENTITY = 0, NRS_TONEMAP_ACES = 1, NRS_TONEMAP_HABLE = 2, NRS_TONEMAP_REINHARD = 3 } nrs_tonemap_curve;
#define NRS_TONEMAP_RGBA32F 0u
#define NRS_TONEMAP_RGBA8 1u
typedef struct nrs_tonemap_params {
	uint32_t struct_size;           /* sizeof(nrs_tonemap_params) */
	float    exposure;              /* m_exposure: the colour is scaled by 2^exposure */
	float    background_color[4];   /* sRGB-encoded, as m_background_color */
	uint32_t color_space;           /* of the accumulate buffer: 0 Linear, 1 SRGB, 2 VisPosNeg (treated as linear) */
	uint32_t output_color_space;    /* 0 Linear, 1 SRGB */
	uint32_t tonemap_curve;         /* 0 Identity, 1 ACES, 2 Hable, 3 Reinhard */
	uint32_t clamp_output;          /* 0 / 1 */
	uint32_t output_format;         /* NRS_TONEMAP_RGBA32F, NRS_TONEMAP_RGBA8 */
} nrs_tonemap_params;
int nrs_tonemap(nrs_ctx* ctx, void* stream, uint32_t width, uint32_t height, const float* d_accumulate, const nrs_tonemap_params* params, void* d_out);
int nrs_accumulate_spp_tonemap(nrs_ctx* ctx, void* stream, uint32_t width, uint32_t height, const float* d_frames, size_t slab_stride_pixels, uint32_t spp_count,
                               float* d_accumulate, uint32_t sample_count, const nrs_tonemap_params* params, void* d_out);
size_t nrs_tonemap_output_bytes(uint32_t width, uint32_t height, uint32_t output_format);

/* ---- mesh extraction: marching cubes on the density field ------------------------------------------------------------------------------------ */
/* Testbed::compute_marching_cubes_mesh / compute_and_save_marching_cubes_mesh (src/python_api.cu:105-127, src/testbed.cu:337-343) = Testbed::marching_cubes
 * (src/testbed_nerf.cu:4614-4649) = get_density_on_grid + marching_cubes_gpu + compute_mesh_1ring + compute_mesh_vertex_colors (src/marching_cubes.cu:730-758, :656-662;
 * src/testbed_nerf.cu:4515-4536), then save_mesh (src/marching_cubes.cu:760-896).  Callers detect these entry points by symbol (dlsym); NRS_ABI_VERSION is unchanged
 * because no existing layout changes.  Not here: the Adam state of the vertices, trainable_verts, optimise_mesh_step, the UV unwrap.
 *
 * The case table is the library's own, generated at first use from a rule: the reference's numbering of corners, edges and mask bits; on a cube face
 * with four crossed edges every SET corner is cut off on its own (the choice depends on the face's corners alone, so both cells of a face agree: no holes); loops over the
 * crossed edges in order of their lowest edge, each fanned from the first edge, walking from the lowest, whose fan has no diagonal inside a cube face; winding such that
 * (pb - pa) x (pa - pc) of a triangle (a, b, c) points out of the dense side, as accumulate_1ring and save_mesh expect.  Vertices are the reference's; which diagonals
 * split a loop, and the pairing on ambiguous faces, are not.
 *
 * Host-only (no context, no GPU):
 * nrs_marching_cubes_res <- get_marching_cubes_res (src/marching_cubes.cu:48-55): float arithmetic in the reference's order, each axis rounded up to a multiple of 16.
 * nrs_marching_cubes_table: *row_len = length of a row (the longest row and its terminator: found by the generator); out (may be NULL) receives [256][*row_len] edge
 *   numbers, three per triangle, terminated by -1.
 * nrs_mesh_write <- save_mesh without its unwrap branch: the extension "ply" selects the ASCII PLY, anything else the OBJ (v with colours, vn, f a//a b//b c//c).  Positions
 *   are written as (v - offset) / scale, normals normalised here (a zero normal stays zero), colour bytes (unsigned char)clamp(c * 255, 0, 255), faces in reversed index
 *   order, the reference's printf formats.  A file that cannot be opened is NRS_ERR_INVALID_ARG with the path in the message.
 *
 * nrs_mesh_from_density <- marching_cubes_gpu + compute_mesh_1ring on the caller's lattice d_density[x + y * rx + z * rx * ry] (what nrs_density_on_grid writes), any res3d
 *   with every axis >= 2.  A vertex sits on a lattice edge whose ends lie on different sides of thresh (f > thresh; a NaN counts as not above), at
 *   (x + dt, y, z) * scale + aabb_min with dt = (thresh - f0) / (f1 - f0) and scale = (aabb_max - aabb_min) / res3d, product and sum separate.  The numbering is
 *   DETERMINISTIC: vertices by ascending (point index, axis), triangles by ascending cell index and table order inside a cell -- one of the numberings the reference's atomic
 *   counters can produce, and the same one every run.  n_verts_padded = (n_verts + 127) & ~127; padding rows are zero.  verts_smoothed (f32x4) and vert_normals (f32x3, not
 *   normalised) are the sums of accumulate_1ring added per vertex in ascending triangle order: bit-reproducible, equal to the sequential sum.  An empty surface is 0 vertices,
 *   0 triangles and a valid handle.  NRS_ERR_INVALID_ARG before any launch, with the argument named: a NULL pointer, an axis < 2, 3 * rx * ry * rz >= 2^31, a non-finite thresh
 *   or box, aabb_max <= aabb_min on an axis.  The call SYNCHRONISES `stream`: once when the counts come back to size the arrays (the reference reads its counters back the
 *   same way) and again before it returns, when its temporaries (4 bytes per lattice point, 4 per vertex) are released.
 * nrs_mesh_extract <- Testbed::marching_cubes: res3d rounded up to multiples of 16 per axis, the lattice evaluated by nrs_density_on_grid's kernel (mask_with_density_grid as
 *   there), the step above, then vertex colours for all n_verts_padded rows: dir = normalize(v - 0.5); network input (warp_position(v, model aabb), warp_dt(MIN_CONE_STEPSIZE),
 *   warp_direction(dir)); the full network with the model's numerics and light direction; network_to_rgb with the model's rgb activation, linear_to_srgb when linear_colors.
 *   nrs_mesh_color_inputs (test hook) writes those [n_verts_padded x 7] inputs of a mesh to d_coords_out.
 * nrs_mesh_counts / _device / _download / _destroy: any out pointer may be NULL; d_colors is NULL for a mesh made by nrs_mesh_from_density (asking _download for its colours
 *   is NRS_ERR_STATE); _download copies the padded rows and n_tris x 3 indices, synchronously. */
typedef struct nrs_mesh nrs_mesh;
int  nrs_marching_cubes_res(uint32_t res_1d, const float aabb_min[3], const float aabb_max[3], uint32_t res3d_out[3]);
int  nrs_marching_cubes_table(int8_t* out, uint32_t* row_len);
int  nrs_mesh_write(const char* path, uint32_t n_verts, const float* h_verts, const float* h_normals, const float* h_colors, uint32_t n_tris, const uint32_t* h_indices,
                    float scale, const float offset[3]);
int  nrs_mesh_from_density(nrs_ctx* ctx, void* stream, const uint32_t res3d[3], const float aabb_min[3], const float aabb_max[3], float thresh, const float* d_density,
                           nrs_mesh** mesh_out);
int  nrs_mesh_extract(nrs_model* model, void* stream, const uint32_t res3d[3], const float aabb_min[3], const float aabb_max[3], float thresh, int mask_with_density_grid,
                      int linear_colors, nrs_mesh** mesh_out);
int  nrs_mesh_color_inputs(nrs_model* model, void* stream, const nrs_mesh* mesh, float* d_coords_out);
int  nrs_mesh_counts(const nrs_mesh* mesh, uint32_t* n_verts, uint32_t* n_verts_padded, uint32_t* n_tris);
int  nrs_mesh_device(const nrs_mesh* mesh, const float** d_verts, const float** d_normals, const float** d_colors, const float** d_smoothed, const uint32_t** d_indices);
int  nrs_mesh_download(const nrs_mesh* mesh, float* h_verts, float* h_normals, float* h_colors, float* h_smoothed, uint32_t* h_indices);
void nrs_mesh_destroy(nrs_mesh* mesh);

/* ---- selection tool: region growing, morphology, the fine mesh -------------------------------------------------------------------------------- */
/* What lies between nrs_project_selection_pixels / nrs_selection_cells (the seed cells) and the cage: RegionGrowing (src/editing/tools/region_growing.cu),
 * CorrectMMOperations (src/editing/tools/correct_mm_operations.cu) and GrowingSelection::dilate / erode / extract_fine_mesh (src/editing/tools/growing_selection.cu:2083-2162).
 * Callers detect these entry points by symbol (dlsym); NRS_ABI_VERSION is unchanged because no existing layout changes.  Not here: the Automatic growing mode (not
 * implemented in the reference either), the proxy cage (progressive hulls), fTetWild, MeshFix.
 *
 * A selection handle holds m_density_grid_host, m_max_cascade, the selection bitfield S (density-bitfield layout: bit morton3D(x, y, z) of level l at byte
 * (l * 128^3 + idx) / 8), the ordered cell list L = m_selection_cell_idx WITH its duplicates, the FIFO queue Q, the growing level g, m_performed_closing and the two
 * structuring elements (dilation Cube 2, erosion Sphere 2: correct_mm_operations.h:70).  Growing is host-only (no context, no GPU): its result depends on pop order.
 *
 * nrs_selection_create: copies h_density_grid; n_floats != 5 * 128^3 or max_cascade > 4 is NRS_ERR_INVALID_ARG.  nrs_selection_destroy releases it.
 * nrs_selection_reset <- reset_growing (region_growing.cu:10-55): S, Q, L cleared; every seed whose level is <= growing_level enters Q and L in input order, lifted
 *   with nrs_upper_cell_idx; higher seeds are dropped; seeds enter L but NOT S; performed_closing cleared.  g := growing_level here already (the reference leaves
 *   m_growing_level to the grow_region that follows, whose caller passes the same value), so the accessors describe the seeds at their level before any growth.  A seed >= 5 * 128^3 or growing_level > 4: NRS_ERR_INVALID_ARG.
 * nrs_selection_grow <- grow_region, Manual mode (:93-141): nothing happens on an empty queue; g := growing_level; at most growing_steps entries are popped (*n_popped,
 *   may be NULL); a popped cell is accepted iff its bit is clear and grid[cell] >= density_threshold and its level is g; an accepted cell on the grid's shell (is_boundary,
 *   selection_utils.cu:8) first upscales the selection (below) and is lifted with it, accepted without a second test; acceptance pushes the up to six neighbours in the order
 *   -x, -y, -z, +x, +y, +z (add_neighbours, :15-34), appends the cell to L and sets its bit.  performed_closing is cleared.  A non-finite density_threshold or
 *   growing_level > 4: NRS_ERR_INVALID_ARG.
 * nrs_selection_upscale <- upscale_selection (:57-91): nothing at g == max_cascade (and at g == 4, the last level there is); else g + 1, S rebuilt from L lifted one
 *   level (L keeps its length and duplicates), every entry of Q lifted.
 * nrs_selection_state: any out pointer may be NULL.  nrs_selection_get_cells: L as cells [n_cells] and / or as points [n_cells x 3] = get_cell_pos (selection_utils.cu:65)
 *   of each cell at its own level, in the reference's float operation order.  nrs_selection_get_bitfield: S [NRS_BITFIELD_BYTES].
 * nrs_selection_set_structuring_elements: type NRS_SE_CUBE (|i|, |j|, |k| <= r) or NRS_SE_SPHERE (i^2 + j^2 + k^2 <= r^2), radius 1..10, for each of the two operations;
 *   anything else is NRS_ERR_INVALID_ARG.
 *
 * nrs_bitfield_morph <- CorrectMMOperations::dilate / erode (correct_mm_operations.cu:117-187) on the device.  op NRS_MORPH_DILATE: a cell of `level` is set iff any
 *   IN-GRID tap of the element is set (hit); NRS_MORPH_ERODE: iff no in-grid tap is clear (fit).  Taps outside the grid are ignored: dilation never wraps, erosion treats the
 *   outside as set, a full grid erodes to a full grid.  d_in and d_out are whole bitfields (NRS_BITFIELD_BYTES, 16-byte aligned, not overlapping); only `level` of d_in is
 *   read; in d_out every other level is ZERO when the call completes, as in the reference.  SCRATCH CONTRACT: the call allocates nothing and is asynchronous on
 *   `stream`; until it completes there, two of d_out's OTHER levels hold its intermediate rows, so no level of d_out may be read or written by other work (another
 *   stream, the host) while the call is in flight -- not even the levels the call only zeroes.  The kernels work on packed words: the level is re-packed to x-major rows, the x extent of each (dy, dz) row of the element is done with
 *   word shifts and carries, rows are combined with OR (on the complement for erosion), and the result is packed back.  NRS_ERR_INVALID_ARG before any launch, with the
 *   argument named: a NULL or misaligned pointer, overlapping bitfields, level > 4, radius outside 1..10, an unknown op or element.
 * nrs_bitfield_morph_host: the same contract on host pointers, as the reference's loops on one thread (a loop over the taps of every cell that ends at the first hit /
 *   miss; a tap is a load from an unpacked copy of the level, not a Morton encode, the taps of one (i, j) column are a run clipped to the grid, and a column of the
 *   grid that holds no set -- for erosion no clear -- cell is passed over): the CPU twin for tests and the baseline of tools/selection_mesh_probe.py.
 * nrs_selection_dilate / _erode <- GrowingSelection::dilate / erode (growing_selection.cu:2083-2093): S := op(S) at level g on the device with the handle's element,
 *   then L is rebuilt from S in the reference's loop order (x outer, y, z inner).  Synchronous.  performed_closing is not touched.
 * nrs_selection_fine_mesh <- extract_fine_mesh (:2096-2162): if use_morphological and not performed_closing: dilate, erode, set the flag.  Then a 128^3 float lattice is
 *   built on the device (x + 128 y + 128^2 z; 1.0 at every cell of L whose level is g and which is not on the grid's shell -- L, not S: without morphology the seeds that
 *   failed the density test are in it, as in the reference) and nrs_mesh_from_density's code runs on it with the box 0.5 +- 0.5 * 2^g, res3d 128, thresh 0.5.  The closed
 *   bitfield does not travel through the host between the closing and the lattice (L and S are still refreshed on the host for the accessors).  The result is an ordinary
 *   nrs_mesh without colours.  Synchronous.  A handle is used with one device: a context on another is NRS_ERR_INVALID_ARG. */
typedef struct nrs_selection nrs_selection;
enum { NRS_SE_CUBE = 0, NRS_SE_SPHERE = 1 };        /* ESEType */
enum { NRS_MORPH_DILATE = 0, NRS_MORPH_ERODE = 1 };
int  nrs_selection_create(const float* h_density_grid, size_t n_floats, uint32_t max_cascade, nrs_selection** sel_out);
void nrs_selection_destroy(nrs_selection* sel);
int  nrs_selection_reset(nrs_selection* sel, const uint32_t* h_cells, uint32_t n, uint32_t growing_level);
int  nrs_selection_grow(nrs_selection* sel, float density_threshold, uint32_t growing_level, uint32_t growing_steps, uint32_t* n_popped);
int  nrs_selection_upscale(nrs_selection* sel);
int  nrs_selection_state(const nrs_selection* sel, uint32_t* growing_level, uint32_t* n_cells, uint32_t* n_queue, int* performed_closing);
int  nrs_selection_get_cells(const nrs_selection* sel, uint32_t* h_cells_out, float* h_points_out);
int  nrs_selection_get_bitfield(const nrs_selection* sel, uint8_t* h_bitfield_out);
int  nrs_selection_set_structuring_elements(nrs_selection* sel, int dilation_type, int dilation_radius, int erosion_type, int erosion_radius);
int  nrs_bitfield_morph(nrs_ctx* ctx, void* stream, const uint8_t* d_in, uint32_t level, int op, int se_type, int radius, uint8_t* d_out);
int  nrs_bitfield_morph_host(const uint8_t* h_in, uint32_t level, int op, int se_type, int radius, uint8_t* h_out);
int  nrs_selection_dilate(nrs_ctx* ctx, void* stream, nrs_selection* sel);
int  nrs_selection_erode(nrs_ctx* ctx, void* stream, nrs_selection* sel);
int  nrs_selection_fine_mesh(nrs_ctx* ctx, void* stream, nrs_selection* sel, int use_morphological, nrs_mesh** mesh_out);

/* ---- training rays: sample generation, the ray loss and its gradient ---------------------------------------------------------------------------- */
/* The two steps between "rays + the colours they should have" and nrs_network_backward: generate_training_samples_nerf (src/testbed_nerf.cu:1087, from :1188 on: everything
 * after the ray exists) and compute_loss_kernel_train_nerf (:1685-1985) with the seven losses of :103-171.  Callers detect these entry points by symbol (dlsym);
 * NRS_ABI_VERSION is unchanged because no existing layout changes.  The rays themselves -- image / pixel selection, lens distortion, rolling shutter -- come from a
 * dataset (nrs_dataset_rays, below) or from the caller.  The envmap and its gradient are nrs_envmap_*'s and nrs_ray_loss_ex's, further down; per-image exposure enters
 * through the target colour alone and is nrs_exposure_*'s, at the end.  Not here: the error map and sharpness, max_level_rand_training, image / pixel PDFs (img_pdf = xy_pdf = 1), fill_rollover_and_rescale
 * (nrs_network_backward takes any n), the camera-gradient kernels, the distill variants, light-direction models.
 *
 * Both calls are asynchronous on `stream`, never wait for the device and keep their per-ray workspace in the model: it is allocated on the first call of a size and
 * reused afterwards (a larger n_rays grows it, which frees the smaller one: hipFree waits for the device).  Because the workspace belongs to the model, two of these calls
 * on ONE model must not be in flight on different streams at the same time.  No float atomics anywhere: two calls with the same inputs give bit-identical outputs.
 *
 * DEVIATIONS from the reference, all deliberate: the ORDER (next paragraph); per-ray arrays in place of the dataset look-ups (nrs_ray_loss); and two guards of the
 * generator's walk against rays it could never end on, which the reference would hang on: a ray whose origin is not finite or whose direction's length lies outside
 * [0.5, 2] has no samples (unit length is otherwise not checked), and a walk gives up after 65 536 empty cells (a ray through the largest box crosses a few thousand).
 *
 * ORDER.  The reference takes a ray's first sample (`base`) and its slot from atomicAdd, so its layout depends on arrival order.  Here both come from an exclusive scan in
 * input order, in both calls; everything else (which rays are kept, what is clipped) follows the reference's rule with the scan's value in place of the atomic's.
 *
 * nrs_training_samples <- :1188-1246.  d_rays [n_rays x 6] f32: origin, direction (unit length expected, not checked).  d_jitter [n_rays] f32 in [0, 1) or NULL for 0:
 *   the reference's random_val(rng).  Per ray: tmin = max(aabb.ray_intersect(o, d).x, 0), startt = tmin + calc_dt(tmin, cone) * jitter, then while the training box contains
 *   o + t d and j < NERF_STEPS (1024): a sample where the cell is occupied at mip_from_dt(dt, pos) (t += dt), advance_to_next_voxel otherwise.  The box and the density
 *   bitfield are the model's.  With j_i the count of ray i: base(i) = the sum of j_k over rays k < i; ray i is emitted iff j_i > 0 and base(i) + j_i <= max_samples
 *   (:1214-1221); emitted rays keep their input order.
 *   d_coords_out [max_samples x ld] f32, ld >= 7: record base + s = warp_position(pos), warp_dt(dt), warp_direction(d) of sample s; floats 7..ld-1 are never written.
 *   Every record from the end of the last emitted ray up to max_samples gets floats 0..6 = 0 (a superset of [min(total, max_samples), max_samples): the gap a dropped ray
 *   leaves is zeroed too), so inference and backward can run on n = max_samples without reading a counter back.
 *   d_numsteps_out [n_rays x 2] u32: (count, base) per EMITTED ray, compact.  d_ray_indices_out [n_rays] u32: the input index of each emitted ray.  Entries at or past the
 *   number of emitted rays are not written.  d_counters [2] u32: [0] rays emitted, [1] the sum of all counts (the reference's numsteps_counter: dropped rays count).
 *   NRS_ERR_INVALID_ARG, before any HIP call: a NULL model / d_coords_out / d_counters / (with n_rays > 0) d_rays / d_numsteps_out / d_ray_indices_out, ld < 7,
 *   max_samples == 0, a non-finite or negative cone_angle_constant, n_rays > 2^21 (2^21 rays of NERF_STEPS samples are 2^31: the 32-bit sample counters).
 *   NRS_ERR_UNSUPPORTED: a model with n_extra_dims != 0.  NRS_ERR_STATE: no density bitfield.
 *   n_rays == 0 is NRS_OK: the counters are zeroed and the records zero-filled.
 *
 * nrs_ray_loss <- :1685-1985.  Inputs: d_numsteps [n_rays x 2] (count, base): bases in any order, with gaps; d_coords [n_samples x ld_in] f32 and d_output_fp16
 *   (planes [16 x ld_out] or interleaved [n_samples x 16], exactly what nrs_network_inference wrote); a ray whose base + count exceeds n_samples, or whose count exceeds NERF_STEPS
 *   (1024), is treated as count 0.
 *   d_ray_counter: u32 on the device, the number of live rays (the generator's d_counters[0]), capped at n_rays; NULL = n_rays.  n_rays itself is the normaliser.  Indexed by
 *   ray slot like d_numsteps (the caller gathers with d_ray_indices_out): d_target_rgba [n_rays x 4] f32, linear and premultiplied (read_rgba); d_background [n_rays x 3],
 *   sRGB-encoded (train_with_random_bg_color), or NULL for params->background; d_ray_origins [n_rays x 3], or NULL when near_distance <= 0.
 *   Per live ray, EPS = 1e-4: the forward composite stops before the first sample with T < EPS (M samples consumed of N); target and background by colour space and
 *   train_in_linear_colors (:1808-1823); if M == N the background is added behind (C += T bg).  cbase(i) = the sum of M_k over live rays k < i,
 *   M' = min(max_samples_compacted - min(max_samples_compacted, cbase), M).  d_numsteps_out [n_rays x 2] = (M', cbase) for live rays (others not written; it must NOT
 *   alias d_numsteps: the gradient pass reads both); *d_counter_out = the sum of M, unclipped.  d_loss [n_rays] (may be NULL) = mean(L) / n_rays, 0 for a ray with
 *   M' == 0 and for rays at or past the counter.  The gradient pass replays samples 0..M'-1 and writes, at compact index cbase + j: d_coords_out = the input record
 *   (ld_in floats) and rows 0..3 of d_dL_doutput_fp16 (planes [16 x ld_dl], ld_dl >= max_samples_compacted, or interleaved [max_samples_compacted x 16]; rows 4..15 are
 *   never written and nrs_network_backward never reads them), round-to-nearest fp16, no clamp:
 *     dL[c] = s (w_j g_c network_to_rgb_derivative(out[c]) + max(0, l2reg out[c])), s = loss_scale / n_rays, l2reg = 1e-4 iff rgb_activation is Exponential;
 *     dL[3] = s network_to_density_derivative(out[3]) dt_j dot(g, T rgb_j - (C - C2)) + (out[3] < 0 ? -l1 : 0) + (out[3] > -10 && |pos_j - origin| < near_distance ? 1e-4 : 0),
 *   with T the transmittance AFTER sample j and C2 the running colour including it (:1910-1916); l1 = 1e-4 iff density_l1_reg; the last two terms are not scaled by s,
 *   as in the reference.  Compact indices [min(sum M, max_samples_compacted), max_samples_compacted) get dL rows 0..3 = 0 and zero records: nrs_network_backward can run
 *   on n = max_samples_compacted without a read-back, and a zero dL contributes nothing to any sum.
 *   NRS_ERR_INVALID_ARG, before any HIP call: a NULL model / params / d_coords_out / d_dL_doutput_fp16 / d_counter_out / (with n_rays > 0) d_numsteps / d_coords /
 *   d_output_fp16 / d_target_rgba / d_numsteps_out, d_numsteps_out == d_numsteps, a struct_size other than sizeof, an unknown loss, colour space or layout, ld_in < 7,
 *   planes with ld_out < n_samples or ld_dl < max_samples_compacted, max_samples_compacted == 0, a non-finite loss_scale, near_distance > 0 with NULL d_ray_origins,
 *   n_rays > 2^21, d_coords_out overlapping d_coords (rays read and write different ranges at the same time: the compaction is not done in place).
 *   n_rays == 0 is NRS_OK (the counter is zeroed, the compact buffers are zero-filled). */
typedef enum nrs_loss_type { NRS_LOSS_L2 = 0, NRS_LOSS_L1 = 1, NRS_LOSS_MAPE = 2, NRS_LOSS_SMAPE = 3, NRS_LOSS_HUBER = 4, NRS_LOSS_LOG_L1 = 5,
                             NRS_LOSS_RELATIVE_L2 = 6 } nrs_loss_type; /* ELossType's order, common.h:96 */
typedef struct nrs_ray_loss_params {
	uint32_t struct_size;            /* refused unless == sizeof(nrs_ray_loss_params) */
	uint32_t loss_type;              /* nrs_loss_type */
	float    loss_scale;
	uint32_t color_space;            /* NRS_COLOR_LINEAR | NRS_COLOR_SRGB */
	uint32_t train_in_linear_colors;
	float    background[3];          /* sRGB-encoded like m_background_color; used when d_background is NULL */
	float    near_distance;          /* <= 0: term off, d_ray_origins may be NULL */
	uint32_t density_l1_reg;         /* the caller's evaluation of *mean_density_ptr < NERF_MIN_OPTICAL_THICKNESS (0.01) */
	uint32_t max_samples_compacted;
} nrs_ray_loss_params;
int nrs_training_samples(nrs_model* model, void* stream, uint32_t n_rays, const float* d_rays, const float* d_jitter, float cone_angle_constant, uint32_t max_samples,
                         float* d_coords_out, uint32_t ld, uint32_t* d_numsteps_out, uint32_t* d_ray_indices_out, uint32_t* d_counters);
int nrs_ray_loss(nrs_model* model, void* stream, const nrs_ray_loss_params* params, uint32_t n_rays, const uint32_t* d_ray_counter, const uint32_t* d_numsteps,
                 uint32_t n_samples, const float* d_coords, uint32_t ld_in, const void* d_output_fp16, uint32_t ld_out, int out_layout, const float* d_target_rgba,
                 const float* d_background, const float* d_ray_origins, uint32_t* d_numsteps_out, float* d_coords_out, void* d_dL_doutput_fp16, uint32_t ld_dl,
                 int dl_layout, float* d_loss, uint32_t* d_counter_out);

/* ---- optimiser: the fused Adam step between nrs_network_backward and the next forward pass ------------------------------------------------------- */
/* The optimiser the reference trains with -- Ema(0.95) over ExponentialDecay(20000, 10000, 0.33) over Adam(1e-2, 0.9, 0.99, 1e-15, l2_reg 1e-6), configs/nerf/base.json,
 * stepped by m_trainer->optimizer_step(stream, LOSS_SCALE) (src/testbed_nerf.cu:3761) -- as one pass over the parameters.  tiny-cuda-nn itself is not part of the
 * reference tree, so THIS TEXT IS THE DEFINITION of the rule (as recalled from tiny-cuda-nn's adam.h); tests/optimizer_ref.py restates it in float64.  Callers detect
 * these entry points by symbol (dlsym); NRS_ABI_VERSION is unchanged because no existing layout changes.  Not here (tiny-cuda-nn's defaults are "off"): AdaBound limits,
 * weight clipping, relative and absolute weight decay.  Non-finite gradients are not filtered, as in tiny-cuda-nn.
 *
 * THE RULE.  n parameters in the blob's order, the first n_matrix of them matrix weights.  Per element i, in fp32 without contraction, in exactly this order:
 *     g = grad[i] / loss_scale
 *     if i >= n_matrix and g == 0:  master, m, v, steps and fp16 of i stay untouched   (the skip; -0 counts as 0: no momentum drift, no step count)
 *     if i <  n_matrix:             g = g + l2_reg * w                                (w = master[i])
 *     m = beta1 * m[i] + (1 - beta1) * g
 *     v = beta2 * v[i] + (1 - beta2) * (g * g)
 *     t = ++steps[i]                                                                  (uint32, one counter per parameter)
 *     lr_i = learning_rate * (i >= n_matrix ? non_matrix_lr_factor : 1) * bias(t)
 *     w' = w - (lr_i / (sqrt(v) + epsilon)) * m
 *     master[i] = w';  fp16[i] = round-to-nearest-even(w')
 *   bias(t) = sqrt(1 - beta2^t) / (1 - beta1^t) comes from a table: the host evaluates it in float64 for t = 1 .. T_sat and rounds each value once to fp32; T_sat is the
 *   first t FROM WHICH ON the rounded value is exactly 1.0f (about 1 650 for base.json's betas; "from which on" because bias(1) is 1 as well whenever
 *   1 - beta2 == (1 - beta1)^2, as with 0.9 / 0.99); the kernel reads table[min(t, T_sat)].  A DEVIATION from tiny-cuda-nn's fp32 powf per element, deliberate: more
 *   accurate, exactly reproducible, and the step stays memory-bound.
 *   EMA, when ema_decay = d > 0: every step and for EVERY element (the skip does not apply) ema[i] = a * ema[i] + b * float(fp16[i]), where with T the optimiser's own
 *   step count after this step a = d (1 - d^(T-1)) / (1 - d^T) and b = (1 - d) / (1 - d^T), computed by the host in float64 and rounded once.  ema is fp32 (tiny-cuda-nn
 *   keeps it in fp16: a deviation).  With ema_decay == 0 the ema array is never touched by a step.
 *   zero_grad != 0: 0.0f is stored to grad[i] wherever a non-zero value (any bit set) was read, so the caller's next nrs_network_backward can run with accumulate = 1
 *   and no memset.
 *
 * nrs_adam_bias_table (host only): out[t - 1] = bias(t) for t = 1 .. T_sat, *n_out = T_sat; `out` may be NULL to ask for the size; NRS_ERR_INVALID_ARG when cap < T_sat
 *   (with out != NULL), for a beta outside [0, 1), and when T_sat would exceed 65 536 (a beta very close to 1).
 * nrs_exponential_decay_lr (host only): base * decay_base^k with k = 0 while steps_done < decay_start, else floor((steps_done - decay_start) / decay_interval) + 1,
 *   evaluated in float64 and rounded once.  decay_interval == 0 counts as 1.  This is the definition (as recalled from tiny-cuda-nn's exponential_decay.h).
 *
 * nrs_optimizer_create: an optimiser over n_params elements with its own fp16 array.  nrs_optimizer_create_for_model: n_params and n_matrix are the model's (all MLP
 *   weights, then the hash table); the fp16 of the hash table is the model's RESIDENT table -- a step writes it in place, no staging and no copy -- the fp16 MLP weights go to
 *   a small buffer of the optimiser's, from which the step re-arranges the MFMA fragments on the same stream (the kernel of nrs_model_set_params_device), and the model's
 *   cell records, if it keeps any, are rebuilt behind that.  The model must outlive the optimiser; while it is bound, nrs_model_set_params / _device on it would put the
 *   fp16 out of step with the master weights (call nrs_optimizer_set_weights instead).  Supported for models without light directions.
 * nrs_optimizer_set_weights: the fp32 master weights from a host (on_device == 0; returns when the copy is done) or device pointer; zeroes m, v, steps and the step
 *   count, sets ema to the weights and writes the fp16 copy (into the model if bound: from then on it has parameters).
 * nrs_optimizer_step: asynchronous on `stream`, never waits for the device.  d_grad [n_params] f32, any 4-byte alignment.
 * nrs_optimizer_get_state / _set_state: synchronous (they wait for the device first); `which` is nrs_optimizer_state, n must be n_params; MASTER / M / V / EMA are f32,
 *   STEPS u32, PARAMS_FP16 u16.  For tests and checkpoints, with nrs_optimizer_step_count / _set_step_count.  set_state on a bound optimiser with PARAMS_FP16 also
 *   refreshes the model's fragments and records.
 * nrs_optimizer_export_fp16: the whole blob as fp16 into d_out [n_params], asynchronous: NRS_OPT_EXPORT_WEIGHTS copies the fp16 the network reads,
 *   NRS_OPT_EXPORT_EMA rounds ema (round to nearest even): what a second model renders with (nrs_model_set_params_device) while the first one trains.
 * Refused before any HIP call.  NRS_ERR_INVALID_ARG: a NULL argument; a struct_size other than sizeof(nrs_adam_params); a beta outside [0, 1); a negative or non-finite
 *   epsilon, l2_reg, learning_rate or non_matrix_lr_factor; a loss_scale that is not finite or <= 0; ema_decay outside [0, 1); n_matrix > n_params; n_params == 0 or
 *   > 2^31; an unknown `which`; n != n_params in get / set.  NRS_ERR_UNSUPPORTED: a model with n_extra_dims != 0.  NRS_ERR_STATE: a step, export or
 *   get / set before nrs_optimizer_set_weights. */
typedef struct nrs_optimizer nrs_optimizer;
typedef struct nrs_adam_params {
	uint32_t struct_size;          /* refused unless == sizeof(nrs_adam_params) */
	float    beta1, beta2;         /* base.json: 0.9, 0.99 */
	float    epsilon;              /* 1e-15 */
	float    l2_reg;               /* 1e-6, matrix weights only */
	float    non_matrix_lr_factor; /* 1 */
	float    ema_decay;            /* 0.95; 0 = no EMA */
} nrs_adam_params;
typedef enum nrs_optimizer_state { NRS_OPT_MASTER = 0, NRS_OPT_M = 1, NRS_OPT_V = 2, NRS_OPT_STEPS = 3, NRS_OPT_EMA = 4, NRS_OPT_PARAMS_FP16 = 5 } nrs_optimizer_state;
typedef enum nrs_optimizer_export { NRS_OPT_EXPORT_WEIGHTS = 0, NRS_OPT_EXPORT_EMA = 1 } nrs_optimizer_export;
int      nrs_adam_bias_table(float beta1, float beta2, float* out, uint32_t cap, uint32_t* n_out);
float    nrs_exponential_decay_lr(float base, uint32_t decay_start, uint32_t decay_interval, float decay_base, uint32_t steps_done);
int      nrs_optimizer_create(nrs_ctx* ctx, size_t n_params, size_t n_matrix, const nrs_adam_params* params, nrs_optimizer** out);
int      nrs_optimizer_create_for_model(nrs_model* model, const nrs_adam_params* params, nrs_optimizer** out);
void     nrs_optimizer_destroy(nrs_optimizer* opt);
int      nrs_optimizer_set_weights(nrs_optimizer* opt, const float* weights_f32, int on_device, void* stream);
int      nrs_optimizer_step(nrs_optimizer* opt, void* stream, float* d_grad, float loss_scale, float learning_rate, int zero_grad);
int      nrs_optimizer_get_state(nrs_optimizer* opt, int which, void* h_out, size_t n);
int      nrs_optimizer_set_state(nrs_optimizer* opt, int which, const void* h_in, size_t n);
int      nrs_optimizer_export_fp16(nrs_optimizer* opt, int which, void* d_out_fp16, void* stream);
uint32_t nrs_optimizer_step_count(const nrs_optimizer* opt);
int      nrs_optimizer_set_step_count(nrs_optimizer* opt, uint32_t steps);
size_t   nrs_optimizer_n_params(const nrs_optimizer* opt, size_t* n_matrix);

/* ---- the dataset: posed images on the device, pixel rays and their targets ------------------------------------------------------------------------- */
/* What stands in front of nrs_training_samples: the first half of generate_training_samples_nerf (src/testbed_nerf.cu:1087-1186: image and pixel selection, the camera
 * of the pixel's time, lens distortion), the look-ups compute_loss_kernel_train_nerf repeats for a ray's target and background (:1777-1806), the loader's image
 * conversion (from_rgba32, common_device.cuh:513-540; from_fullp, src/nerf_loader.cu:62) and mark_untrained_density_grid (:353-400).  Callers detect these entry
 * points by symbol (dlsym); NRS_ABI_VERSION is unchanged because no existing layout changes.  The error-map CDFs (cdf_img, cdf_x_cond_y) are
 * nrs_dataset_rays_ex's, further down: nrs_dataset_rays is the `cdf == nullptr` branches.  Not here: explicit per-pixel rays (rays_in), the trainable per-pixel distortion map (the envmap is nrs_envmap_*'s and per-image exposure nrs_exposure_*'s, further down), light directions (a dataset serves
 * n_extra_dims == 0 models), sharpening and the sharpness map, EXR, the adaptive rays_per_batch of train_nerf (it reads counters back), decoding image files (the
 * Python package does that).
 *
 * A dataset owns n_images images of one resolution, stored as the reference stores them (NerfDataset::images_data): fp16 RGBA, linear, premultiplied, 8 bytes per pixel,
 * image after image, rows top to bottom -- a ray reads its pixel in one 64-bit load -- and one camera record per image.  A dataset is used from one host thread and its
 * calls on ONE stream at a time (the staging buffer of host pixels and the camera block are the dataset's own).
 *
 * nrs_dataset_set_image: `pixels` is width x height pixels of `format`, a host pointer or (is_device_pointer != 0) a device pointer; asynchronous on `stream` for device
 *   pixels, host pixels have been read when it returns (they travel through a staging buffer of the dataset, allocated once).
 *   NRS_IMAGE_RGBA8_SRGB  <- from_rgba32<__half>: alpha = a * (1 / 255), colour = srgb_to_linear(c * (1 / 255)) * alpha with srgb_to_linear(s) = s / 12.92 for
 *     s <= 0.04045, else powf((s + 0.055) / 1.055, 2.4), rounded to fp16 once.  NRS_IMAGE_WHITE_TRANSPARENT / _BLACK_TRANSPARENT: a pixel whose colour bytes are all 255 /
 *     all 0 gets alpha 0.  A pixel whose four bytes, read as a little-endian word, equal a non-zero mask_color becomes (-1, -1, -1, -1): masked away.
 *   NRS_IMAGE_RGBA32F_LINEAR <- from_fullp: each float rounded to fp16 (flags and mask_color are ignored).  NRS_IMAGE_RGBA16F_LINEAR: copied as it is.
 * nrs_dataset_get_image: image `index` as the dataset holds it, width x height x 4 halves to the host; synchronous (it waits for the device first).  For tests and checkpoints.
 *   NRS_ERR_STATE while that image has never been set.
 * nrs_dataset_set_camera: xform_start / xform_end are 3 x 4 column-major like nrs_render_params::camera_matrix0 (the camera at pixel time 0 / 1), focal_length in pixels,
 *   principal_point in [0, 1]^2 (screen_center), rolling_shutter, distortion_mode (0 none, 1 iterative, 2 f-theta) and distortion_params as in nrs_render_params.  The
 *   records stay on the host until a device call needs them and then travel in one block (that call waits for the copy).
 *
 * nrs_dataset_rays: one thread per ray i, outputs in input order, in the reference's order and float32 expressions:
 *   img = (((i + n_rays_total) * n_images) / n_rays) % n_images in 32-bit unsigned arithmetic (image_idx, :1072; the product wraps as the reference's does);
 *   the generator pcg32 (rng_state, rng_inc: nrs_rng_seed) advanced by 8 i (N_MAX_RANDOM_SAMPLES_PER_RAY); draws 0 and 1 are xy, draw 2 motionblur_time, draw 3 the
 *   jitter; the background is draws 2, 3 and 4 -- what the loss kernel gets when it re-seeds and draws three floats behind xy (:1780-1791; max_level_rand_training is off
 *   everywhere in this library);  snap_to_pixel_centers as :1047;  the pixel is image_pos (:1075: multiply, truncate, clamp);  target_rgba = the pixel's four halves as
 *   float (read_rgba);  the camera is start + (end - start) * pixel_t, pixel_t = rs.x + rs.y u + rs.z v + rs.w motionblur_time (get_xform_given_rolling_shutter,
 *   common_device.cuh:226 -- NOT the render path's blend);  the direction is :1169-1185: f_theta_undistortion with error direction (0, 0, 1), or
 *   ((xy - pp) * res / focal, 1) with iterative_camera_undistortion in mode 1, then xform.block<3, 3>(0, 0) * d, normalised.
 *   A masked pixel (first channel < 0, :1127) makes a DEAD ray: direction (0, 0, 0), origin the camera's, target 0; jitter, background and pixel are written as for any
 *   ray.  nrs_training_samples gives such a ray no samples (its length guard), so it is never emitted and never gathered.
 *   Outputs: d_rays [n x 6] f32, d_jitter [n] f32, d_target_rgba [n x 4] f32, d_background [n x 3] f32 (sRGB-encoded, as nrs_ray_loss expects it; written only when
 *   random_bg_color, NULL allowed otherwise), d_pixels [n x 2] u32 (img, x + y * width) or NULL.  Two calls with the same inputs give bit-identical outputs.
 * nrs_dataset_mark_untrained <- mark_untrained_density_grid on the model's float density grid, all five cascades: a cell that no camera sees (the start transform, the
 *   frustum test widened by the voxel radius; an f-theta camera counts as "sees everything") gets -1, a seen cell gets 0 under the reference's condition
 *   (clear_visible_voxels, or the cell's sign disagrees with what was found); then mean, bitfield and mips are rebuilt as nrs_model_set_density_grid rebuilds them
 *   (the call waits for the stream there, like every bitfield rebuild).  nrs_model_update_density_grid keeps negative cells negative.
 * nrs_rng_advance (host only): pcg32's skip-ahead, *state moved by `delta` steps of the generator (state, inc).  The reference advances m_rng once per training step
 *   (src/testbed_nerf.cu:4435) by tiny-cuda-nn's default delta, which is not in the reference tree: NRS_RNG_STEP_DELTA = 2^32 is the value used here (pcg32::advance's
 *   default argument as recalled from tiny-cuda-nn's pcg32.h; the occupancy refresh already steps by it).
 *
 * Refused before any HIP call, NRS_ERR_INVALID_ARG: NULL handles or outputs; an index past n_images; a zero resolution or n_images == 0; an unknown format or distortion
 *   mode; a wrong struct_size; a non-finite camera entry or a focal length that is not positive; n_rays > 2^21 (the generator's own limit); a dataset and a model of
 *   different contexts.  NRS_ERR_STATE: nrs_dataset_rays or nrs_dataset_mark_untrained while an image or a camera has never been set.  n_rays == 0 is NRS_OK. */
typedef struct nrs_dataset nrs_dataset;
typedef enum nrs_image_format { NRS_IMAGE_RGBA8_SRGB = 0, NRS_IMAGE_RGBA32F_LINEAR = 1, NRS_IMAGE_RGBA16F_LINEAR = 2 } nrs_image_format;
#define NRS_IMAGE_WHITE_TRANSPARENT 1u
#define NRS_IMAGE_BLACK_TRANSPARENT 2u
#define NRS_RNG_STEP_DELTA (1ull << 32)
typedef struct nrs_training_camera {
	uint32_t struct_size;          /* refused unless == sizeof(nrs_training_camera) */
	float    xform_start[12];      /* TrainingXForm::start, column-major 3 x 4 */
	float    xform_end[12];        /* TrainingXForm::end */
	float    focal_length[2];      /* pixels */
	float    principal_point[2];   /* fraction of the image */
	float    rolling_shutter[4];
	uint32_t distortion_mode;      /* 0 none, 1 iterative (k1 k2 p1 p2), 2 f-theta (p0..p4, w, h) */
	float    distortion_params[7];
} nrs_training_camera;
typedef struct nrs_dataset_rays_params {
	uint32_t struct_size;          /* refused unless == sizeof(nrs_dataset_rays_params) */
	uint32_t n_rays_total;         /* rays generated by the steps before this one (m_nerf.training.n_rays_total) */
	uint64_t rng_state, rng_inc;   /* m_rng for this step */
	uint32_t snap_to_pixel_centers;
	uint32_t random_bg_color;
} nrs_dataset_rays_params;
int  nrs_dataset_create(nrs_ctx* ctx, uint32_t n_images, uint32_t width, uint32_t height, nrs_dataset** out);
void nrs_dataset_destroy(nrs_dataset* ds);
int  nrs_dataset_set_image(nrs_dataset* ds, uint32_t index, int format, const void* pixels, int is_device_pointer, uint32_t flags, uint32_t mask_color, void* stream);
int  nrs_dataset_set_camera(nrs_dataset* ds, uint32_t index, const nrs_training_camera* camera);
int  nrs_dataset_get_image(nrs_dataset* ds, uint32_t index, void* h_out_fp16);
int  nrs_dataset_rays(nrs_dataset* ds, void* stream, const nrs_dataset_rays_params* params, uint32_t n_rays, float* d_rays, float* d_jitter, float* d_target_rgba,
                      float* d_background, uint32_t* d_pixels);
int  nrs_dataset_mark_untrained(nrs_model* model, nrs_dataset* ds, int clear_visible_voxels, void* stream);
void nrs_rng_advance(uint64_t* state, uint64_t inc, uint64_t delta);

/* ---- the training error map: accumulate, CDFs, rays sampled in proportion to it ---------------------------------------------------------------------- */
/* The error map of train_nerf (src/testbed_nerf.cu:3724-3831): every ray's loss is deposited into a small per-image map (:1861-1886), the map is turned into three
 * CDFs (construct_cdf_2d :2620, construct_cdf_1d :2650, the host loop :3811-3822), and the next steps' images and pixels are drawn from them (image_idx :1052,
 * sample_cdf_2d :983).  All of it is state of an nrs_dataset and runs on the device with nothing read back; all of it is new surface, detected by symbol
 * (nrs_dataset_rays_ex); nrs_dataset_rays and nrs_ray_loss are what they were.  Not here: the sharpness map and include_sharpness_in_error (:1872-1881).
 *
 * THREE DEVIATIONS, all deliberate:
 *  1. The cells are unsigned 64-bit fixed point, not floats: no float atomic on the training path, and two calls give the same bits.  A deposit v (float32) is
 *     skipped unless v > 0 (that also drops NaN); otherwise it adds (uint64)(min(v, 1024.f) * 4294967296.f) -- the product is exact, the conversion truncates, the
 *     add is one no-return 64-bit integer atomic.  Integer sums do not depend on the order of arrival, so the map, the CDFs and every ray drawn from them are
 *     reproducible.  2^21 deposits of the clamp value fit without a wrap.  The float map the reference keeps is (float)cell * 2^-32, formed where it is read.
 *  2. The deposit is e = (loss[slot] * n_rays) / pdf with loss[slot] the per-slot mean nrs_ray_loss wrote.  The reference divides each channel's loss by the pdf and
 *     then averages (:1848, :1856): a few float32 roundings apart.  The map steers sampling; it is part of no gradient (nor is the pdf, in the reference: :1850-1854).
 *  3. The map's resolution lies in [2, min(image resolution, 1024)] on each axis.  At resolution 1 the reference's own deposit writes cell x + 1 outside the map; with
 *     the map no finer than the image, the reference's clamp of the cell index by the IMAGE resolution (:1866) never acts: the position is already clamped to
 *     res - (1 + 1e-4), so the cell is at most res - 2.  (The kernel clamps the cell into [0, res - 2] for the sake of a NaN in d_xy; for every other input that is
 *     the same cell.)
 *
 * nrs_dataset_error_map_reset: (re)allocates and zeroes n_images x res_y x res_x cells (:3724-3728), asynchronous on `stream` (a reallocation waits for the device).
 *   Valid CDFs carry their own resolution (cdf_resolution beside resolution) and survive.
 * nrs_error_map_resolution (host only): one axis of the reference's choice, (int)(sqrtf(sqrtf((float)((steps_between * rays_per_batch) / n_images))) * 3.5f) with the
 *   product in 32-bit unsigned arithmetic, clamped into [2, min(image_resolution, 1024)]; 0 when n_images == 0 or image_resolution < 2 (no map is possible).
 * nrs_dataset_error_map_set: the map from res_y x res_x x n_images floats of the host, each quantised by the deposit rule (what it skips is 0).  Synchronous.
 * nrs_dataset_error_map_get: `what` to the host, synchronous; *count (may be NULL) receives the number of elements, h_out may be NULL to ask for the count alone.
 *   NRS_ERROR_MAP_FLOAT: (float)cell * 2^-32 [n_images][res_y][res_x] f32;  NRS_ERROR_MAP_CELLS: the cells, uint64;  NRS_ERROR_MAP_CDF_X_COND_Y [n_images][res_y][res_x],
 *   _CDF_Y [n_images][res_y], _CDF_IMG [n_images], _PMF_IMG [n_images]: f32, at the CDFs' resolution.  For tests, checkpoints and display.
 * nrs_dataset_error_map_accumulate: one thread per ray slot s < min(*d_ray_counter, n_rays).  i = d_ray_indices[s] (nrs_training_samples), img = d_pixels[2 i],
 *   xy = d_xy[2 i ..], p = d_pdf ? d_pdf[i] : 1, e = (d_loss[s] * (float)n_rays) / p, then :1862-1886: pos = clamp(xy * res - 0.5, 0, res - (1 + 1e-4f)), truncated to
 *   the cell, the fraction is the weight, four bilinear products (1 - wx) * (1 - wy) * e ... evaluated left to right, each deposited by rule 1.  d_loss_weighted (NULL,
 *   or it may alias d_loss) receives d_loss[s] / p: the loss the reference reports (:1848).  A slot whose loss is 0 deposits nothing (the early return at :1838).
 *   A slot whose ray index is not below n_rays or whose image is not below n_images is skipped.
 * nrs_dataset_error_map_build_cdfs: per (image, row) the running sum of data[x] + 1e-10f in ascending x, the row's total into cdf_y, then
 *   (1.0f - 0.01f) * c * (1.0f / total) + 0.01f * (float)(x + 1) / (float)width;  the same over a picture's rows (no 1e-10f), the total into cdf_img;  over the images
 *   with MIN_PMF = 0.1f: pmf_img = (1.0f - 0.1f) * total * norm + 0.1f / n_images, cdf_img likewise with (float)(i + 1) / n_images.  IEEE division, no contraction,
 *   products and sums in the written order; THE SERIAL ASSOCIATION OF EACH RUNNING SUM IS PART OF THE DEFINITION.  Records the CDFs' resolution and marks them valid.
 * nrs_error_map_cdfs_host (host only): the same expressions on the host, data = the float map; outputs sized as nrs_dataset_error_map_get lays them out.
 *
 * nrs_dataset_rays_ex: nrs_dataset_rays with two switches and two more outputs, d_xy [n x 2] f32 (xy after snapping: what the accumulate needs) and d_pdf [n] f32 =
 *   img_pdf * xy_pdf (either may be NULL).  With both switches off every output it shares with nrs_dataset_rays has that call's bits and the pdf is exactly 1.  The
 *   generator's draw order is the same under every switch -- no draw is added -- so jitter, background and motion-blur time keep their bits.
 *   binary_search (common.h:187-210): the first index whose entry is not < val, capped at length - 1.
 *   sample_images_by_error (image_idx, :1052-1064): img = binary_search(ld_random_val(i + n_rays_total, 0xdeadbeef), cdf_img, n_images), img_pdf = (cdf_img[img] - prev)
 *     * n_images.
 *   sample_pixels_by_error (sample_cdf_2d, :983-1012, on draws 0 and 1): x < 0.5f is the uniform half, x /= 0.5f and xy_pdf stays 1.  Otherwise x = (x - 0.5f) /
 *     (1.0f - 0.5f); the row comes from cdf_y and y = (y - prev) / pmf_y; the column from that row of cdf_x_cond_y and x = (x - prev) / pmf_x; xy_pdf = pmf_x * pmf_y *
 *     (res_x * res_y); xy = ((float)col + x) / res_x, ((float)row + y) / res_y.  xy_pdf is the density of the CDF half ALONE, not the mixture's (pdf_2d, :1014): that
 *     is what the reference divides by, and it is kept.  Then snap_to_pixel_centers and everything behind it as in nrs_dataset_rays.
 *
 * Refused before any HIP call, NRS_ERR_INVALID_ARG: NULL handles, a wrong struct_size, NULL inputs or outputs that are required, a resolution outside
 *   [2, min(image resolution, 1024)], an unknown `what`, n_rays > 2^21.  NRS_ERR_STATE: accumulate, get (map or cells), build_cdfs without a map; get of a CDF and
 *   nrs_dataset_rays_ex with a switch on without valid CDFs; nrs_dataset_rays_ex while an image or a camera has never been set. */
typedef enum nrs_error_map_what {
	NRS_ERROR_MAP_FLOAT = 0, NRS_ERROR_MAP_CDF_X_COND_Y = 1, NRS_ERROR_MAP_CDF_Y = 2, NRS_ERROR_MAP_CDF_IMG = 3, NRS_ERROR_MAP_PMF_IMG = 4, NRS_ERROR_MAP_CELLS = 5
} nrs_error_map_what;
#define NRS_ERROR_MAP_MAX_RESOLUTION 1024u
typedef struct nrs_dataset_rays_ex_params {
	uint32_t struct_size;          /* refused unless == sizeof(nrs_dataset_rays_ex_params) */
	uint32_t n_rays_total;
	uint64_t rng_state, rng_inc;
	uint32_t snap_to_pixel_centers;
	uint32_t random_bg_color;
	uint32_t sample_images_by_error;   /* sample_image_proportional_to_error */
	uint32_t sample_pixels_by_error;   /* sample_focal_plane_proportional_to_error */
} nrs_dataset_rays_ex_params;
int      nrs_dataset_error_map_reset(nrs_dataset* ds, uint32_t res_x, uint32_t res_y, void* stream);
uint32_t nrs_error_map_resolution(uint32_t steps_between, uint32_t rays_per_batch, uint32_t n_images, uint32_t image_resolution);
int      nrs_dataset_error_map_set(nrs_dataset* ds, uint32_t res_x, uint32_t res_y, const float* h_data_f32);
int      nrs_dataset_error_map_get(nrs_dataset* ds, int what, void* h_out, size_t* count);
int      nrs_dataset_error_map_accumulate(nrs_dataset* ds, void* stream, uint32_t n_rays, const uint32_t* d_ray_counter, const uint32_t* d_ray_indices, const float* d_loss,
                                          const float* d_xy, const uint32_t* d_pixels, const float* d_pdf, float* d_loss_weighted);
int      nrs_dataset_error_map_build_cdfs(nrs_dataset* ds, void* stream);
int      nrs_error_map_cdfs_host(uint32_t n_images, uint32_t res_y, uint32_t res_x, const float* data, float* cdf_x_cond_y, float* cdf_y, float* cdf_img, float* pmf_img);
int      nrs_dataset_rays_ex(nrs_dataset* ds, void* stream, const nrs_dataset_rays_ex_params* params, uint32_t n_rays, float* d_rays, float* d_jitter, float* d_target_rgba,
                             float* d_background, uint32_t* d_pixels, float* d_xy, float* d_pdf);

/* ---- image metrics: PSNR and SSIM of a rendered view against a held-out image, on the device --------------------------------------------------------- */
/* What scripts/run.py --test_transforms prints (:215-302; linear_to_srgb / srgb_to_linear scripts/common.py:139-145, luminance and SSIM :186-207, compute_error_img
 * :227-247, compute_error :264-269), as one stencil-and-reduce kernel over the accumulate buffer and the reference image where it lies.  New surface, detected by
 * symbol (nrs_image_metrics).  Not here: MAE, MAPE, SMAPE, MRSE, FLIP, per-frame fovs of a test file, EXR references.
 *
 * THE DEFINITION.  I: the rendered image, f32x4 per pixel, linear, rows top to bottom (the accumulate buffer after its folds); only rgb is read.  Rf: the reference,
 * NRS_IMAGE_RGBA16F_LINEAR (a dataset image as nrs_dataset stores it: linear, premultiplied) or NRS_IMAGE_RGBA32F_LINEAR of the same meaning.  Per pixel, float32,
 * IEEE division, no contraction, products and sums in the written order; powf is the platform's (the device library's, glibc's in the host twin):
 *  1. the reference.  color_space == NRS_COLOR_SRGB (NeRF's blend in sRGB space, run.py:264-270), with a = Rf.w:  c = a != 0 ? Rf.rgb / a : 0;
 *     c = linear_to_srgb(c) * a + (1.0f - a) * background_color.rgb;  ref = srgb_to_linear(c).  Any other colour space: ref = Rf.rgb.  (run.py sets the background
 *     (0, 0, 0, 1).)  linear_to_srgb(l) = l > 0.0031308f ? 1.055f * powf(l, 0.41666667f) - 0.055f : 12.92f * l  and  srgb_to_linear(s) = s > 0.04045f ?
 *     powf((s + 0.055f) / 1.055f, 2.4f) : s / 12.92f -- run.py's curves, NOT nrs_tonemap's (`<`, 0.41666).
 *  2. A = clip(linear_to_srgb(I.rgb)) and R = clip(linear_to_srgb(ref)) with clip(x) = x < 0 ? 0 : (x > 1 ? 1 : x); then a non-finite A (a NaN: the clip passes it)
 *     counts as 0 (compute_error_img :228-229).
 *  3. squared error: e_c = (A_c - R_c) * (A_c - R_c) for c = r, g, b; a non-finite e_c (a NaN in the reference) counts as 0 (compute_error :266).
 *  4. SSIM.  La = (0.2126f * powf(A.r, g) + 0.7152f * powf(A.g, g)) + 0.0722f * powf(A.b, g) with g = 0.4545454545f, Lb likewise from R: yes, on top of the sRGB
 *     encoding -- the reference's quirk, kept.  blur is the separable 5-tap kernel k = (0.120078f, 0.233881f, 0.292082f, 0.233881f, 0.120078f), along y first, then
 *     along x, one axis being v[0] + (k[1] * ((v[-1] - v[0]) + (v[1] - v[0])) + k[0] * ((v[-2] - v[0]) + (v[2] - v[0]))): the centre's weight is 1 - 2 k[1] - 2 k[0]
 *     = 0.292082 exactly, so this is the 5-tap sum with weights that add up to one, and a constant neighbourhood comes back bit for bit.  The boundary is scipy's `reflect`: index i of an axis of length n
 *     reads j = i mod 2n (the non-negative remainder), j < n ? j : 2n - 1 - j -- for n = 1 and 2 as well.  mA = blur(La), mB = blur(Lb), sA = blur(La * La) - mA * mA,
 *     sB = blur(Lb * Lb) - mB * mB, sAB = blur(La * Lb) - mA * mB,
 *       ssim = ((2.0f * mA * mB + 1e-4f) / ((mA * mA + mB * mB) + 1e-4f)) * ((2.0f * sAB + 9e-4f) / ((sA + sB) + 9e-4f)),  non-finite -> 0.
 *  5. the sums, exact and order-free (the error map's convention): every e_c and every pixel's ssim is multiplied by 2^32 (exact) and rounded to the nearest integer
 *     (ties to even; ssim is signed); these are summed as 64-bit integers, on the device with ONE no-return 64-bit integer atomic per sum and workgroup.  A view's
 *     record is bit-identical from run to run and does not depend on the tile shape or the order of arrival.  8192^2 pixels x 3 x 2^32 < 2^63.
 *  6. the record: mse = sum_sq_err * 2^-32 / (3 n) and ssim = sum_ssim * 2^-32 / n, each evaluated in double and rounded to float once; psnr = -10 * log10(mse) from
 *     the rounded mse, in double, rounded once; +inf for mse == 0.
 * A masked dataset pixel (-1, -1, -1, -1) gets NO special case: it is computed as its stored values say (in NRS_COLOR_LINEAR its R is 0; a test set has no masks).
 *
 * nrs_image_metrics: three things on `stream` -- a 16-byte clear of the two sums, the kernel, a one-thread kernel that fills n_pixels, mse, ssim, psnr -- nothing waits
 *   for the device, nothing is allocated.  d_image 16-byte aligned, d_reference 8-byte (fp16) / 16-byte (f32) aligned, d_result 8-byte aligned.  d_ssim_map and
 *   d_sq_err_map (either may be NULL): float [height x width], the pixel's ssim and (e_r + e_g + e_b) / 3.0f -- run.py's metric maps.
 * nrs_dataset_image_metrics: the reference is image `index` of the dataset, read in place; width and height are the dataset's, the context is the dataset's.
 *   NRS_ERR_STATE while that image has never been set.
 * nrs_image_metrics_host: the CPU twin on host pointers -- the same float32 operations in the same order, the same fixed-point sums, glibc's powf.  No context, no GPU.
 * nrs_image_metrics_summary_host: run.py's totals over n records (:292-301), in double: psnr_mean, psnr_min, psnr_max (plain minimum and maximum of the records'
 *   psnr; run.py's starting values 1000 and 0 are not kept), ssim_mean, psnr_avgmse = -10 * log10(mean mse) (+inf for 0).
 *
 * Refused before any HIP call, NRS_ERR_INVALID_ARG: NULL handles, inputs or result; a zero dimension or one above NRS_IMAGE_METRICS_MAX_DIM; a struct_size other than
 *   sizeof(nrs_image_metrics_params); a reference_format other than the two above (NRS_IMAGE_RGBA8_SRGB included); a non-finite background; a misaligned pointer; an
 *   index past n_images; n == 0 records. */
#define NRS_IMAGE_METRICS_MAX_DIM 8192u
typedef struct nrs_image_metrics_params {
	uint32_t struct_size;          /* refused unless == sizeof(nrs_image_metrics_params) */
	uint32_t color_space;          /* nrs_color_space of the training: NRS_COLOR_SRGB blends the reference in sRGB space (step 1) */
	float    background_color[4];  /* sRGB-encoded; run.py: (0, 0, 0, 1) */
	uint32_t reference_format;     /* NRS_IMAGE_RGBA16F_LINEAR | NRS_IMAGE_RGBA32F_LINEAR */
} nrs_image_metrics_params;
typedef struct nrs_image_metrics_result {
	int64_t  sum_sq_err;           /* sum of round(e_c * 2^32) over pixels and channels */
	int64_t  sum_ssim;             /* sum of round(ssim * 2^32) over pixels */
	uint32_t n_pixels;
	float    mse, ssim, psnr;
} nrs_image_metrics_result;
typedef struct nrs_metrics_summary {
	double   psnr_mean, psnr_min, psnr_max, ssim_mean, psnr_avgmse;
	uint32_t n_views, reserved;
} nrs_metrics_summary;
int nrs_image_metrics(nrs_ctx* ctx, void* stream, uint32_t width, uint32_t height, const float* d_image, const void* d_reference, const nrs_image_metrics_params* params,
                      nrs_image_metrics_result* d_result, float* d_ssim_map, float* d_sq_err_map);
int nrs_dataset_image_metrics(nrs_dataset* ds, uint32_t index, void* stream, const float* d_image, const nrs_image_metrics_params* params, nrs_image_metrics_result* d_result,
                              float* d_ssim_map, float* d_sq_err_map);
int nrs_image_metrics_host(uint32_t width, uint32_t height, const float* h_image, const void* h_reference, const nrs_image_metrics_params* params,
                           nrs_image_metrics_result* h_result, float* h_ssim_map, float* h_sq_err_map);
int nrs_image_metrics_summary_host(const nrs_image_metrics_result* h_results, uint32_t n, nrs_metrics_summary* out);

/* ---- the environment map: a trained background behind the last sample ------------------------------------------------------------------------------ */
/* The m_envmap the reference trains next to the network (src/testbed.cu:2427-2441, configs/nerf/base.json:76-103): the background a training ray sees
 * (src/testbed_nerf.cu:1792-1801), its gradient (:1961-1984) and its own optimiser step (:3731-3733, :3766-3768).  What it learns is what nrs_render_params::d_envmap
 * reads.  All of it is new surface, detected by symbol (nrs_envmap_create); nrs_ray_loss, nrs_training_samples, nrs_dataset_rays* and nrs_optimizer_* are what they
 * were.  Per-image exposure and its gradient (:1803, :1946-1959) are nrs_exposure_*'s, below.  Not here: loading envmap.png, the equirectangular reader, the distill kernels, light-direction
 * models.  A DELIBERATE OMISSION: rays with zero samples are still not emitted by nrs_training_samples.  The reference's train_envmap switch (:1214) emits them, but
 * its loss kernel returns at :1838 for a ray without compact samples before it reaches the envmap's gradient: the switch changes which slots exist and no gradient.
 *
 * An nrs_envmap owns res_x x res_y RGBA float texels, laid out like d_envmap ([res_y][res_x][4], >= 1 x 1; a lookup wraps in x and clamps in y), an unbound
 * optimiser over its 4 * res_x * res_y floats with n_matrix = 0 (THE RULE of the optimiser block, every texel channel a non-matrix parameter: a channel whose
 * gradient is zero is not touched, the EMA advances for all), a float gradient of that size and a gradient accumulator of signed 64-bit cells.  The default
 * Adam parameters (params == NULL, or what nrs_envmap_default_adam_params fills in) are base.json's envmap block: beta 0.9 / 0.99, epsilon 1e-10, ema_decay 0.99,
 * non_matrix_lr_factor 1; l2_reg is irrelevant because there are no matrix weights.  The learning-rate schedule is the caller's: base.json's is 1e-2 with
 * nrs_exponential_decay_lr(1e-2, 10000, 5000, 0.33, step).  A FRESH MAP IS ALL ZEROS until texels are set (this library's rule: the reference's initial values
 * are tiny-cuda-nn's, which is not part of the reference tree).  The training loss reads the LIVE texels (the optimiser's master weights); rendering and evaluation
 * use the EMA (params() versus params_inference()).  As everywhere in the optimiser the EMA follows the fp16 copy of the weights (a deviation stated there).
 *
 * nrs_envmap_create / _destroy; nrs_envmap_resolution.  Creation allocates everything and waits for the device once; there is no lazy state, so no call here returns
 *   NRS_ERR_STATE.
 * nrs_envmap_set_texels: the live texels from a host (on_device == 0; returns when the copy is done) or device pointer, [res_y][res_x][4] f32; resets the optimiser as
 *   nrs_optimizer_set_weights does (the EMA becomes the texels) and zeroes the gradient and the cells.
 * nrs_envmap_get: synchronous (waits for the device first), n = 4 * res_x * res_y elements to the host.  NRS_ENVMAP_TEXELS: the live texels; NRS_ENVMAP_EMA; NRS_ENVMAP_GRADIENT:
 *   (float)((double)cell * 2^-32) of the cells as they are now, f32 -- the gradient the next step will read (zero right after a step); NRS_ENVMAP_CELLS: the cells, int64.
 * nrs_envmap_export: asynchronous; the live (ema == 0) or the EMA texels into d_out [res_y][res_x][4] f32 on the device: what d_envmap takes.
 *
 * nrs_envmap_background: one thread per ray slot s < min(*d_ray_counter, n_rays).  i = d_ray_indices[s] (nrs_training_samples; a slot with i >= n_rays is skipped),
 *   d = d_rays[6 i + 3 ..], looked up in the live texels by the render path's read_envmap (envmap.cuh:30-63: theta = acosf(clamp(d.y)), phi = atan2f(-d.x, d.z),
 *   f = (phi / 2pi + 0.5, theta / pi) * (res - 1), t = (int)f, w = f - t, bilinear in the order ((w00 a + w10 b) + w01 c) + w11 e).  Two records per slot:
 *     d_background_linear[3 s ..] = env.rgb + srgb_to_linear(bg) * (1 - env.a), bg = d_background[3 s ..] (by slot, sRGB-encoded, as nrs_ray_loss takes it) or
 *       default_background[3] when d_background is NULL; srgb_to_linear is the ray loss's (a division and powf);
 *     d_footprint[4 s ..] = (tx, ty as int32, wx, wy as float32 bits): the texel and the weights of that lookup BEFORE wrapping and clamping; 16-byte aligned.
 *   Slots at or past the counter are not written.  The footprint is computed once per ray and step and handed to the gradient pass (the reference's
 *   deposit_envmap_gradient repeats acosf / atan2f), which also makes that pass a function of integers and float32 products alone.
 *
 * nrs_ray_loss_ex: nrs_ray_loss with two optional additions, both behind null checks where a ray is finished; the walk over the samples is the same code.
 *   d_background_linear [n_rays x 3] f32 by slot replaces srgb_to_linear(d_background / params->background); everything after that line is unchanged.
 *   d_ray_aux [n_rays x 12] 32-bit words by slot, 16-byte aligned, written for live rays: words 0..2 g (loss_and_gradient's gradient), 3 T behind the ray's last
 *   sample, 4..6 the target, 7..9 C (the colour the loss saw, background included), 10 n (u32: the ray's effective count, 0 where nrs_ray_loss treats it as 0),
 *   11 M (u32).  With both NULL every output has nrs_ray_loss's bits; nrs_ray_loss IS that call.
 *
 * nrs_envmap_accumulate <- :1961-1983, one thread per slot s < min(*d_ray_counter, n_rays).  A slot deposits iff d_numsteps_out[2 s] == aux.n && aux.n > 0: the ray has
 *   samples and was neither stopped (M < n) nor clipped by the compact buffer (M' < M).  Then, in fp32 without contraction, in this order:
 *     lg = aux.g, or, if params->envmap_loss_type != params->loss_type, loss_and_gradient(envmap_loss_type, aux.target, aux.C) per channel (the reference's own
 *       envmap loss is RelativeL2, testbed.cu:2438; nrs_envmap_accumulate_params has no default: the caller names both);
 *     dbg = aux.T * lg;   unless train_in_linear_colors:  dbg = dbg / srgb_to_linear_derivative(linear_to_srgb(d_background_linear[3 s + c])) with
 *       srgb_to_linear_derivative(x) = x <= 0.04045f ? 1.0f / 12.92f : 2.4f / 1.055f * powf((x + 0.055f) / 1.055f, 1.4f) (the loss saw the background sRGB-encoded);
 *     v[c] = (loss_scale / (float)n_rays) * dbg[c];   alpha's gradient is 0 as in the reference (:1981): alpha texels never move.
 *   DEPOSIT (the error map's rule, signed): the four weights (1 - wx) * (1 - wy), wx * (1 - wy), (1 - wx) * wy, wx * wy of the slot's footprint; for each weight and
 *   channel p = v[c] * w; skipped unless p is finite and non-zero; clamped to +-512; multiplied by 2^32 (exact); rounded to nearest, ties to even, into int64; added
 *   with ONE no-return 64-bit integer atomic to channel c of texel (wrap(tx + dx), clamp(ty + dy)) -- wrap adds or subtracts res_x once, as the lookup does, and then
 *   clamps into the map, which acts for a footprint no lookup wrote alone.  2^21 rays of the clamp value sum to 2^62: a cell never wraps.
 *   TWO DEVIATIONS, both deliberate: the reference rounds v and the weight to fp16 and adds with float (or half2) atomics; here nothing is rounded to fp16 (the
 *   fixed-point step 2^-32 is finer than fp16's at every magnitude) and the sum does not depend on the order of arrival: two calls give the same bits.
 * nrs_envmap_step: asynchronous, reads nothing back.  One kernel writes gradient[i] = (float)((double)cell[i] * 2^-32) and zeroes every cell it read non-zero; then the
 *   optimiser's step kernel runs on the texels with that gradient, loss_scale, learning_rate and zero_grad = 1.
 *
 * Refused before any HIP call, NRS_ERR_INVALID_ARG: NULL handles or required pointers (with n_rays > 0); a wrong struct_size; a resolution < 1 or with
 *   4 * res_x * res_y > 2^31; n_rays > 2^21; an unknown loss type or `which`; n != 4 * res_x * res_y in get; a misaligned d_footprint / d_ray_aux; a loss_scale that is
 *   not finite (or, for the step, <= 0); a negative or non-finite learning_rate; adam params the optimiser refuses.  No entry point takes both an envmap and a model,
 *   so there is no context mismatch to refuse here.  n_rays == 0 is NRS_OK. */
typedef struct nrs_envmap nrs_envmap;
typedef enum nrs_envmap_what { NRS_ENVMAP_TEXELS = 0, NRS_ENVMAP_EMA = 1, NRS_ENVMAP_GRADIENT = 2, NRS_ENVMAP_CELLS = 3 } nrs_envmap_what;
#define NRS_RAY_AUX_WORDS 12u
typedef struct nrs_envmap_accumulate_params {
	uint32_t struct_size;            /* refused unless == sizeof(nrs_envmap_accumulate_params) */
	uint32_t loss_type;              /* the step's nrs_loss_type: what aux.g was computed with */
	uint32_t envmap_loss_type;       /* the envmap's own; the reference: NRS_LOSS_RELATIVE_L2 */
	float    loss_scale;
	uint32_t train_in_linear_colors;
} nrs_envmap_accumulate_params;
void     nrs_envmap_default_adam_params(nrs_adam_params* out);
int      nrs_envmap_create(nrs_ctx* ctx, uint32_t res_x, uint32_t res_y, const nrs_adam_params* params, nrs_envmap** out);
void     nrs_envmap_destroy(nrs_envmap* envmap);
int      nrs_envmap_resolution(const nrs_envmap* envmap, uint32_t* res_x, uint32_t* res_y);
int      nrs_envmap_set_texels(nrs_envmap* envmap, const float* texels_f32, int on_device, void* stream);
int      nrs_envmap_get(nrs_envmap* envmap, int which, void* h_out, size_t n);
int      nrs_envmap_export(nrs_envmap* envmap, int ema, float* d_out, void* stream);
int      nrs_envmap_background(nrs_envmap* envmap, void* stream, uint32_t n_rays, const uint32_t* d_ray_counter, const uint32_t* d_ray_indices, const float* d_rays,
                               const float* d_background, const float* default_background, float* d_background_linear, int32_t* d_footprint);
int      nrs_ray_loss_ex(nrs_model* model, void* stream, const nrs_ray_loss_params* params, uint32_t n_rays, const uint32_t* d_ray_counter, const uint32_t* d_numsteps,
                         uint32_t n_samples, const float* d_coords, uint32_t ld_in, const void* d_output_fp16, uint32_t ld_out, int out_layout, const float* d_target_rgba,
                         const float* d_background, const float* d_ray_origins, uint32_t* d_numsteps_out, float* d_coords_out, void* d_dL_doutput_fp16, uint32_t ld_dl,
                         int dl_layout, float* d_loss, uint32_t* d_counter_out, const float* d_background_linear, uint32_t* d_ray_aux);
int      nrs_envmap_accumulate(nrs_envmap* envmap, void* stream, const nrs_envmap_accumulate_params* params, uint32_t n_rays, const uint32_t* d_ray_counter,
                               const uint32_t* d_numsteps_out, const uint32_t* d_ray_aux, const float* d_background_linear, const int32_t* d_footprint);
int      nrs_envmap_step(nrs_envmap* envmap, void* stream, float loss_scale, float learning_rate);
uint32_t nrs_envmap_step_count(const nrs_envmap* envmap);

/* ---- per-image exposure: a trained brightness per training view ------------------------------------------------------------------------------------ */
/* m_nerf.training.optimize_exposure (testbed.h:590, off by default; exposure_l2_reg 0 at :593, n_steps_between_cam_updates 16 at :563; the per-image
 * AdamOptimizer<Array3f>(1e-3f) of src/testbed.cu:2309, adam_optimizer.h:38-45): three log2 exposures per training image, trained next to the network.  Exposure
 * enters ONLY through the target colour: exposure_scale = exp(0.6931471805599453f * exposure[img]) multiplies the premultiplied rgb of the target texel in both colour
 * branches of src/testbed_nerf.cu:1808-1823, so handing nrs_ray_loss_ex a pre-scaled target (scale * rgb, a) is the reference's expression, with the product
 * rounded once in fp32; and its gradient (:1946-1959) needs nothing beyond what nrs_ray_loss_ex writes into the ray's aux record.  All of it is new surface,
 * detected by symbol (nrs_exposure_create); NRS_ABI_VERSION is unchanged because no existing layout changes, and nrs_ray_loss_ex is used as it is.  A training view
 * is DISPLAYED with nrs_tonemap_params::exposure = m_exposure + exposure[view] (src/testbed.cu:2808; one value per view: the tonemap takes a scalar, so a caller with
 * three different channels picks one or their mean).  Not here: the distortion map, camera extrinsics, focal length (they need the ray-direction gradients).
 *
 * An nrs_exposure owns n_images x 3 float exposures (ALL ZERO WHEN FRESH: scale 1), Adam first and second moments of that size, ONE step count shared by all images,
 * n_images x 3 signed 64-bit fixed-point gradient cells (2^-32 per unit, the envmap's) and a host-side count of the rays accumulated since the last step.
 * The parameters -- params == NULL, or what nrs_exposure_default_params fills in -- are nrs_exposure_params: beta1 0.9, beta2 0.99, epsilon 1e-8 (adam_optimizer.h:24), l2_reg 0
 * (exposure_l2_reg), steps_between_updates 16 (n_steps_between_cam_updates: the number of training steps whose gradients one nrs_exposure_step averages).
 *
 * nrs_exposure_create / _destroy / _n_images / _step_count.  Creation allocates everything, zeroes it and waits for the device once.
 * nrs_exposure_set: the exposures from the host, [n_images][3] f32, or all zeros (h_values == NULL); resets the moments, the step count, the cells and the ray count
 *   (the reference's per-frame reset_state).  Returns when the copy is done.
 * nrs_exposure_get: synchronous (waits for the device first), n = 3 * n_images elements to the host.  NRS_EXPOSURE_VALUES, _M, _V: f32; NRS_EXPOSURE_CELLS: int64;
 *   NRS_EXPOSURE_GRADIENT: (float)((double)cell * 2^-32) of the cells as they are now, f32 (zero right after a step).
 * nrs_exposure_export: asynchronous; the exposures into d_out [n_images][3] f32 on the device.
 *
 * nrs_exposure_targets <- :1803-1823, one thread per ray slot s < min(*d_ray_counter, n_rays).  d_pixels [n_rays x 2] u32 (img, pixel) BY RAY INDEX, as
 *   nrs_dataset_rays writes it; d_target_rgba [n_rays x 4] f32 by ray index; d_target_out [n_rays x 4] f32 BY SLOT (what nrs_ray_loss_ex takes as d_target_rgba);
 *   d_scale [n_rays x 4] 32-bit words by slot, 16-byte aligned.  i = d_ray_indices[s], img = d_pixels[2 i]; a slot with i >= n_rays or img >= n_images is SKIPPED:
 *   nothing is written for it and it never deposits (nrs_exposure_accumulate skips i >= n_rays itself and reads the slot's d_scale record as the caller left it: a
 *   caller whose batches can hold an img >= n_images fills d_scale with 0xff bytes, or zeros, beforehand -- an img word >= n_images is skipped, a zero scale adds 0).
 *     scale[c] = expf(0.6931471805599453f * exposure[3 img + c]);   d_target_out[4 s ..] = (scale * rgb, a) of d_target_rgba[4 i ..];   d_scale[4 s ..] = (scale.xyz
 *     as f32 bits, img).  One pass replaces the gather of the target by slot.  The scale is computed once per ray and step and handed to the gradient pass, not
 *     recomputed (the envmap's footprint follows the same rule), so that pass is a function of float32 products alone.
 * nrs_exposure_accumulate <- :1946-1959, one thread per slot s < min(*d_ray_counter, n_rays).  A slot that nrs_exposure_targets would not skip deposits iff
 *   d_numsteps_out[2 s] > 0 (the reference returns at :1838 otherwise).  A STOPPED RAY STILL DEPOSITS, unlike the envmap's rule.  With i = d_ray_indices[s],
 *   (scale, img) = d_scale[4 s ..] and aux the slot's nrs_ray_loss_ex record, in fp32 without contraction, in this order:
 *     dgt[c] = -aux.g[c] / pdf,  pdf = d_xy_pdf ? d_xy_pdf[i] : 1 (by ray index; the reference's `/ xy_pdf`, :1948);
 *     unless train_in_linear_colors:  dgt[c] = dgt[c] / srgb_to_linear_derivative(aux.target[c])  (the aux record's target is the sRGB-encoded one there; the
 *       derivative is the envmap block's);
 *     v[c] = (((loss_scale / (float)n_rays) * dgt[c]) * scale[c]) * 0.6931471805599453f   (`/ n_rays`: :1889).
 *   DEPOSIT (the envmap's rule, the same code): v[c] skipped unless finite and non-zero; clamped to +-512; multiplied by 2^32 (exact); rounded to nearest, ties to even,
 *   into int64; added to cell 3 img + c.  THE SUM IS FORMED PER WAVE FIRST: image_idx (:1072) hands out images in runs of consecutive ray indices and slots keep the
 *   input order, so the 64 lanes of a wave almost always share one image.  Each lane quantises; the wave then peels its distinct images one at a time (a ballot of
 *   the lanes left, the image of the first of them broadcast), sums the quantised values of that image's lanes across the wave and issues ONE no-return 64-bit
 *   integer atomic per image, channel and wave (none for a zero sum).  Integer sums do not depend on their order: the cells hold the bits one atomic per lane would
 *   leave, and two calls give the same bits.  DEVIATION: the reference adds floats with atomicAdd; nothing here depends on the order of arrival.
 *   The call adds n_rays to the handle's ray count; the call that would take the count past 2^21 is refused with NRS_ERR_STATE before any HIP call (2^21 rays of the
 *   clamp value sum to 2^62: a cell never wraps).  nrs_exposure_step and nrs_exposure_set reset the count.
 * nrs_exposure_step <- :3885-3911, asynchronous, reads nothing back; one kernel of one workgroup.  Per image and channel, in fp32 in adam_optimizer.h's order:
 *     g = (float)((double)cell * 2^-32) * pcls + value * l2_reg,   pcls = (float)n_images / loss_scale / (float)steps_between_updates on the host (:3838);
 *     m = beta1 * m + (1 - beta1) * g;   v = beta2 * v + (1 - beta2) * (g * g);   value -= alr * (m / (sqrtf(v) + epsilon)).
 *   AN IMAGE WITHOUT RAYS STILL STEPS (g = value * l2_reg, the moments decay, the value moves by momentum), as in the reference -- unlike the network optimiser's
 *   zero-gradient skip (the optimiser block's RULE).  alr = learning_rate * sqrt(1 - beta2^t) / (1 - beta1^t) with the incremented step count t, evaluated in float64
 *   on the host and rounded once: A DEVIATION (the reference uses float std::pow; nrs_exponential_decay_lr deviates in the same way).  Then the renormalisation
 *   (:3900-3909):  mean[c] = (float)(sum_i (double)value[i][c] / (double)n_images), the float64 sum in ONE fixed order, the kernel's and the host twin's (two calls give the same
 *   bits): 1024 strided partial sums, partial j adding the images j, j + 1024, ... in rising order, then the partials in rising order -- up to 1024 images that is
 *   the images in their order;
 *   value[i][c] -= mean[c].  The cells are zeroed and the ray count reset.  ONE STEP COUNT IS SHARED BY ALL IMAGES: A DEVIATION (the reference keeps one optimiser per
 *   image, and they only diverge through its per-frame reset_state, which is nrs_exposure_set here).  learning_rate is the caller's: the reference passes the network
 *   optimiser's current one (m_optimizer->learning_rate(), :3897).
 * nrs_exposure_step_host: the step's host twin on caller arrays, built from the same arithmetic as the kernel (one header, read by both): cells [3 n_images] int64,
 *   values, m, v [3 n_images] f32 and *step_count are read and written in place (cells become zero, *step_count is incremented).  No device, no handle.
 *
 * Refused before any HIP call, NRS_ERR_INVALID_ARG: NULL handles or required pointers (with n_rays > 0); a wrong struct_size; n_images == 0 or above 2^20; betas
 *   outside [0, 1); a non-positive or non-finite epsilon or loss_scale; a negative or non-finite l2_reg or learning_rate; steps_between_updates == 0; n_rays > 2^21;
 *   an unknown `which`; n != 3 * n_images in get; a misaligned d_scale or d_ray_aux; d_target_out aliasing d_target_rgba.  n_rays == 0 is NRS_OK (and counts no rays). */
typedef struct nrs_exposure nrs_exposure;
typedef enum nrs_exposure_what { NRS_EXPOSURE_VALUES = 0, NRS_EXPOSURE_M = 1, NRS_EXPOSURE_V = 2, NRS_EXPOSURE_CELLS = 3, NRS_EXPOSURE_GRADIENT = 4 } nrs_exposure_what;
#define NRS_EXPOSURE_MAX_IMAGES (1u << 20)
typedef struct nrs_exposure_params {
	uint32_t struct_size;            /* refused unless == sizeof(nrs_exposure_params) */
	float    beta1, beta2, epsilon;  /* 0.9, 0.99, 1e-8 */
	float    l2_reg;                 /* exposure_l2_reg: 0 */
	uint32_t steps_between_updates;  /* n_steps_between_cam_updates: 16 */
} nrs_exposure_params;
typedef struct nrs_exposure_accumulate_params {
	uint32_t struct_size;            /* refused unless == sizeof(nrs_exposure_accumulate_params) */
	float    loss_scale;             /* the ray loss's */
	uint32_t train_in_linear_colors; /* the ray loss's */
} nrs_exposure_accumulate_params;
void     nrs_exposure_default_params(nrs_exposure_params* out);
int      nrs_exposure_create(nrs_ctx* ctx, uint32_t n_images, const nrs_exposure_params* params, nrs_exposure** out);
void     nrs_exposure_destroy(nrs_exposure* exposure);
uint32_t nrs_exposure_n_images(const nrs_exposure* exposure);
uint32_t nrs_exposure_step_count(const nrs_exposure* exposure);
int      nrs_exposure_set(nrs_exposure* exposure, const float* h_values);
int      nrs_exposure_get(nrs_exposure* exposure, int which, void* h_out, size_t n);
int      nrs_exposure_export(nrs_exposure* exposure, float* d_out, void* stream);
int      nrs_exposure_targets(nrs_exposure* exposure, void* stream, uint32_t n_rays, const uint32_t* d_ray_counter, const uint32_t* d_ray_indices, const uint32_t* d_pixels,
                              const float* d_target_rgba, float* d_target_out, uint32_t* d_scale);
int      nrs_exposure_accumulate(nrs_exposure* exposure, void* stream, const nrs_exposure_accumulate_params* params, uint32_t n_rays, const uint32_t* d_ray_counter,
                                 const uint32_t* d_ray_indices, const uint32_t* d_numsteps_out, const uint32_t* d_ray_aux, const uint32_t* d_scale, const float* d_xy_pdf);
int      nrs_exposure_step(nrs_exposure* exposure, void* stream, float loss_scale, float learning_rate);
int      nrs_exposure_step_host(uint32_t n_images, const nrs_exposure_params* params, float loss_scale, float learning_rate, int64_t* cells, float* values, float* m,
                                float* v, uint32_t* step_count);

#ifdef __cplusplus
}
#endif
#endif /* NRS_H */
