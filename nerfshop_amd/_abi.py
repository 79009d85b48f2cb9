"""ctypes mirror of include/nrs.h (the C-ABI of the render path) and the loader of libnrs.so.

The library is the product: hand-written HIP kernels for gfx950 + the C++ host code around them.  There is
no CPU fallback anywhere in this package -- if the shared library is missing, `load()` raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NRS_LIB_PATH") or os.path.join(_HERE, "csrc", "libnrs.so")  # NRS_LIB_PATH: A/B builds while profiling

NRS_OK = 0
GRID_SIZE = 128
GRID_CASCADES = 5
GRID_VOLUME = GRID_SIZE ** 3
BITFIELD_BYTES = GRID_VOLUME * GRID_CASCADES // 8
N_LUT_CELLS = GRID_VOLUME * GRID_CASCADES

ACT_NONE, ACT_RELU, ACT_LOGISTIC, ACT_EXPONENTIAL = 0, 1, 2, 3
RENDER_AO, RENDER_SHADE, RENDER_NORMALS, RENDER_POSITIONS, RENDER_DEPTH, RENDER_DISTANCE, RENDER_STEPSIZE, RENDER_DISTORTION, RENDER_COST, RENDER_SLICE = range(10)
RENDER_ENCODING_VIS = 11
LAYOUT_PLANES, LAYOUT_INTERLEAVED = 0, 1


class ModelDesc(C.Structure):
    _fields_ = [
        ("n_levels", C.c_uint32),
        ("n_features_per_level", C.c_uint32),
        ("log2_hashmap_size", C.c_uint32),
        ("base_resolution", C.c_uint32),
        ("per_level_scale", C.c_float),
        ("n_neurons", C.c_uint32),
        ("density_hidden_layers", C.c_uint32),
        ("density_output_dims", C.c_uint32),
        ("rgb_hidden_layers", C.c_uint32),
        ("sh_degree", C.c_uint32),
        ("rgb_activation", C.c_uint32),
        ("density_activation", C.c_uint32),
        ("aabb_min", C.c_float * 3),
        ("aabb_max", C.c_float * 3),
    ]


class TetMesh(C.Structure):
    _fields_ = [
        ("n_vertices", C.c_uint32),
        ("n_tets", C.c_uint32),
        ("h_vertices", C.c_void_p),
        ("h_original_vertices", C.c_void_p),
        ("h_tets", C.c_void_p),
        ("h_lut_offsets", C.c_void_p),
        ("h_lut_idx", C.c_void_p),
        ("h_original_bitfield", C.c_void_p),
        ("h_local_rotations", C.c_void_p),
        ("copy", C.c_uint32),
        ("apply_poisson", C.c_uint32),
        ("residual_amplitude", C.c_float),
        ("h_boundary_shs", C.c_void_p),
        ("h_boundary_outside_density", C.c_void_p),
        ("h_boundary_residual_density", C.c_void_p),
        ("correct_direction", C.c_uint32),
    ]


class AffineDuplicationOp(C.Structure):
    _fields_ = [
        ("selection_center", C.c_float * 3),
        ("selection_scale", C.c_float * 3),
        ("selection_rot", C.c_float * 9),
        ("translation", C.c_float * 3),
        ("scale", C.c_float * 3),
        ("rotation", C.c_float * 9),
        ("hide_original", C.c_uint32),
        ("correct_dir", C.c_uint32),
    ]


class RenderParams(C.Structure):
    """nrs_render_params; struct_size is filled in on construction (NRS_RENDER_PARAMS_INIT)."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("resolution", C.c_int32 * 2),
        ("focal_length", C.c_float * 2),
        ("camera_matrix0", C.c_float * 12),
        ("camera_matrix1", C.c_float * 12),
        ("rolling_shutter", C.c_float * 4),
        ("screen_center", C.c_float * 2),
        ("render_aabb_min", C.c_float * 3),
        ("render_aabb_max", C.c_float * 3),
        ("spp_index", C.c_uint32),
        ("snap_to_pixel_centers", C.c_uint32),
        ("min_transmittance", C.c_float),
        ("cone_angle_constant", C.c_float),
        ("render_mode", C.c_uint32),
        ("linear_colors", C.c_uint32),
        ("apply_operators", C.c_uint32),
        ("poisson_target", C.c_uint32),
        ("min_mip", C.c_uint32),
        ("max_march_steps", C.c_uint32),
        ("tile_size", C.c_uint32),
        ("tile_first", C.c_uint32),
        ("tile_stride", C.c_uint32),
        ("dof", C.c_float),
        ("slice_plane_z", C.c_float),
        ("depth_scale", C.c_float),
        ("show_accel", C.c_uint32),
        ("distortion_mode", C.c_uint32),
        ("distortion_params", C.c_float * 7),
        ("d_distortion_map", C.c_void_p),
        ("distortion_resolution", C.c_int32 * 2),
        ("envmap_resolution", C.c_int32 * 2),
        ("d_envmap", C.c_void_p),
        ("glow_mode", C.c_uint32),
        ("glow_y_cutoff", C.c_float),
        ("visualized_layer", C.c_uint32),
        ("visualized_dimension", C.c_uint32),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_size = C.sizeof(RenderParams)


class RenderStats(C.Structure):
    _fields_ = [("n_samples", C.c_uint64), ("n_rays_alive", C.c_uint32), ("n_rays_hit", C.c_uint32)]


class GridUpdate(C.Structure):
    _fields_ = [
        ("n_uniform_samples", C.c_uint32),
        ("n_nonuniform_samples", C.c_uint32),
        ("reset_grid", C.c_uint32),
        ("max_cascade", C.c_uint32),
        ("decay", C.c_float),
        ("ema_step", C.c_uint32),
        ("rng_state", C.c_uint64),
        ("rng_inc", C.c_uint64),
    ]


class TonemapParams(C.Structure):
    """nrs_tonemap_params; struct_size is filled in on construction."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("exposure", C.c_float),
        ("background_color", C.c_float * 4),
        ("color_space", C.c_uint32),
        ("output_color_space", C.c_uint32),
        ("tonemap_curve", C.c_uint32),
        ("clamp_output", C.c_uint32),
        ("output_format", C.c_uint32),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_size = C.sizeof(TonemapParams)


class SampleView(C.Structure):
    """nrs_sample_view: the view of one sample of nrs_render_nerf_spp_views"""
    _fields_ = [("camera_matrix0", C.c_float * 12), ("camera_matrix1", C.c_float * 12), ("focal_length", C.c_float * 2), ("dof", C.c_float), ("slice_plane_z", C.c_float)]


class CameraKeyframe(C.Structure):
    """nrs_camera_keyframe: R is the quaternion (x, y, z, w)"""
    _fields_ = [("R", C.c_float * 4), ("T", C.c_float * 3), ("slice", C.c_float), ("scale", C.c_float), ("fov", C.c_float), ("dof", C.c_float)]


LOSS_L2, LOSS_L1, LOSS_MAPE, LOSS_SMAPE, LOSS_HUBER, LOSS_LOG_L1, LOSS_RELATIVE_L2 = range(7)  # nrs_loss_type (ELossType's order)


class RayLossParams(C.Structure):
    """nrs_ray_loss_params; the defaults are Testbed's (L2, loss scale 128, Linear, train_in_linear_colors off)"""
    _fields_ = [("struct_size", C.c_uint32), ("loss_type", C.c_uint32), ("loss_scale", C.c_float), ("color_space", C.c_uint32), ("train_in_linear_colors", C.c_uint32),
                ("background", C.c_float * 3), ("near_distance", C.c_float), ("density_l1_reg", C.c_uint32), ("max_samples_compacted", C.c_uint32)]

    def __init__(self, **kw):
        super().__init__()
        self.struct_size = C.sizeof(RayLossParams)
        self.loss_type, self.loss_scale, self.color_space, self.train_in_linear_colors = LOSS_L2, 128.0, 0, 0
        for k, v in kw.items():
            if k == "background":
                self.background = (C.c_float * 3)(*[float(x) for x in v])
            elif k in dict(self._fields_):
                setattr(self, k, v)
            else:
                raise TypeError(f"RayLossParams has no field {k}")


class AdamParams(C.Structure):
    """nrs_adam_params; the defaults are the optimiser of configs/nerf/base.json (Adam 0.9 / 0.99 / 1e-15, l2_reg 1e-6, Ema 0.95)"""
    _fields_ = [("struct_size", C.c_uint32), ("beta1", C.c_float), ("beta2", C.c_float), ("epsilon", C.c_float), ("l2_reg", C.c_float),
                ("non_matrix_lr_factor", C.c_float), ("ema_decay", C.c_float)]

    def __init__(self, **kw):
        super().__init__()
        self.struct_size = C.sizeof(AdamParams)
        self.beta1, self.beta2, self.epsilon, self.l2_reg, self.non_matrix_lr_factor, self.ema_decay = 0.9, 0.99, 1e-15, 1e-6, 1.0, 0.95
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError(f"AdamParams has no field {k}")
            setattr(self, k, v)


def envmap_adam_params():
    """The optimiser of base.json's envmap block (nrs_envmap_default_adam_params): Adam 0.9 / 0.99 / 1e-10, Ema 0.99; l2_reg never acts (no matrix weights)"""
    return AdamParams(epsilon=1e-10, l2_reg=0.0, ema_decay=0.99)


class EnvmapAccumulateParams(C.Structure):
    """nrs_envmap_accumulate_params; struct_size is filled in on construction, the envmap's own loss defaults to the reference's RelativeL2 (testbed.cu:2438)"""
    _fields_ = [("struct_size", C.c_uint32), ("loss_type", C.c_uint32), ("envmap_loss_type", C.c_uint32), ("loss_scale", C.c_float), ("train_in_linear_colors", C.c_uint32)]

    def __init__(self, loss_type=LOSS_L2, envmap_loss_type=LOSS_RELATIVE_L2, loss_scale=128.0, train_in_linear_colors=0):
        super().__init__()
        self.struct_size = C.sizeof(EnvmapAccumulateParams)
        self.loss_type, self.envmap_loss_type, self.loss_scale, self.train_in_linear_colors = int(loss_type), int(envmap_loss_type), float(loss_scale), int(train_in_linear_colors)


class ExposureParams(C.Structure):
    """nrs_exposure_params; the defaults are the reference's per-image AdamOptimizer (0.9 / 0.99 / 1e-8), exposure_l2_reg 0 and n_steps_between_cam_updates 16"""
    _fields_ = [("struct_size", C.c_uint32), ("beta1", C.c_float), ("beta2", C.c_float), ("epsilon", C.c_float), ("l2_reg", C.c_float), ("steps_between_updates", C.c_uint32)]

    def __init__(self, **kw):
        super().__init__()
        self.struct_size = C.sizeof(ExposureParams)
        self.beta1, self.beta2, self.epsilon, self.l2_reg, self.steps_between_updates = 0.9, 0.99, 1e-8, 0.0, 16
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError(f"ExposureParams has no field {k}")
            setattr(self, k, v)


class ExposureAccumulateParams(C.Structure):
    """nrs_exposure_accumulate_params; struct_size is filled in on construction"""
    _fields_ = [("struct_size", C.c_uint32), ("loss_scale", C.c_float), ("train_in_linear_colors", C.c_uint32)]

    def __init__(self, loss_scale=128.0, train_in_linear_colors=0):
        super().__init__()
        self.struct_size = C.sizeof(ExposureAccumulateParams)
        self.loss_scale, self.train_in_linear_colors = float(loss_scale), int(train_in_linear_colors)


class TrainingCamera(C.Structure):
    """nrs_training_camera; struct_size is filled in on construction.  Matrices are 3 x 4 column-major like RenderParams.camera_matrix0."""
    _fields_ = [("struct_size", C.c_uint32), ("xform_start", C.c_float * 12), ("xform_end", C.c_float * 12), ("focal_length", C.c_float * 2),
                ("principal_point", C.c_float * 2), ("rolling_shutter", C.c_float * 4), ("distortion_mode", C.c_uint32), ("distortion_params", C.c_float * 7)]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_size = C.sizeof(TrainingCamera)


class DatasetRaysParams(C.Structure):
    """nrs_dataset_rays_params; struct_size is filled in on construction."""
    _fields_ = [("struct_size", C.c_uint32), ("n_rays_total", C.c_uint32), ("rng_state", C.c_uint64), ("rng_inc", C.c_uint64), ("snap_to_pixel_centers", C.c_uint32),
                ("random_bg_color", C.c_uint32)]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_size = C.sizeof(DatasetRaysParams)


class DatasetRaysExParams(C.Structure):
    """nrs_dataset_rays_ex_params; struct_size is filled in on construction."""
    _fields_ = [("struct_size", C.c_uint32), ("n_rays_total", C.c_uint32), ("rng_state", C.c_uint64), ("rng_inc", C.c_uint64), ("snap_to_pixel_centers", C.c_uint32),
                ("random_bg_color", C.c_uint32), ("sample_images_by_error", C.c_uint32), ("sample_pixels_by_error", C.c_uint32)]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_size = C.sizeof(DatasetRaysExParams)


# nrs_error_map_what
ERROR_MAP_FLOAT, ERROR_MAP_CDF_X_COND_Y, ERROR_MAP_CDF_Y, ERROR_MAP_CDF_IMG, ERROR_MAP_PMF_IMG, ERROR_MAP_CELLS = 0, 1, 2, 3, 4, 5
ERROR_MAP_MAX_RESOLUTION = 1024  # NRS_ERROR_MAP_MAX_RESOLUTION


IMAGE_RGBA8_SRGB, IMAGE_RGBA32F_LINEAR, IMAGE_RGBA16F_LINEAR = 0, 1, 2  # nrs_image_format
IMAGE_METRICS_MAX_DIM = 8192  # NRS_IMAGE_METRICS_MAX_DIM


class ImageMetricsParams(C.Structure):
    """nrs_image_metrics_params; struct_size is filled in on construction, the background is run.py's (0, 0, 0, 1), the reference fp16."""
    _fields_ = [("struct_size", C.c_uint32), ("color_space", C.c_uint32), ("background_color", C.c_float * 4), ("reference_format", C.c_uint32)]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_size = C.sizeof(ImageMetricsParams)
        if "background_color" not in kw and len(args) < 3:
            self.background_color[:] = (0.0, 0.0, 0.0, 1.0)
        if "reference_format" not in kw and len(args) < 4:
            self.reference_format = IMAGE_RGBA16F_LINEAR


class ImageMetricsResult(C.Structure):
    """nrs_image_metrics_result: 32 bytes, METRICS_RECORD_DTYPE as a numpy record"""
    _fields_ = [("sum_sq_err", C.c_int64), ("sum_ssim", C.c_int64), ("n_pixels", C.c_uint32), ("mse", C.c_float), ("ssim", C.c_float), ("psnr", C.c_float)]


class MetricsSummary(C.Structure):
    """nrs_metrics_summary"""
    _fields_ = [("psnr_mean", C.c_double), ("psnr_min", C.c_double), ("psnr_max", C.c_double), ("ssim_mean", C.c_double), ("psnr_avgmse", C.c_double),
                ("n_views", C.c_uint32), ("reserved", C.c_uint32)]


METRICS_RECORD_DTYPE = [("sum_sq_err", "<i8"), ("sum_ssim", "<i8"), ("n_pixels", "<u4"), ("mse", "<f4"), ("ssim", "<f4"), ("psnr", "<f4")]
IMAGE_WHITE_TRANSPARENT, IMAGE_BLACK_TRANSPARENT = 1, 2  # NRS_IMAGE_WHITE_TRANSPARENT / _BLACK_TRANSPARENT
RNG_STEP_DELTA = 1 << 32  # NRS_RNG_STEP_DELTA
OPT_MASTER, OPT_M, OPT_V, OPT_STEPS, OPT_EMA, OPT_PARAMS_FP16 = range(6)  # nrs_optimizer_state
OPT_EXPORT_WEIGHTS, OPT_EXPORT_EMA = 0, 1  # nrs_optimizer_export
# the schedule of configs/nerf/base.json: ExponentialDecay(decay_start, decay_interval, decay_base) over a learning rate of 1e-2
BASE_LEARNING_RATE, BASE_DECAY_START, BASE_DECAY_INTERVAL, BASE_DECAY_BASE = 1e-2, 20000, 10000, 0.33
# the schedule of its envmap block: ExponentialDecay(10000, 5000, 0.33) over 1e-2
ENVMAP_LEARNING_RATE, ENVMAP_DECAY_START, ENVMAP_DECAY_INTERVAL, ENVMAP_DECAY_BASE = 1e-2, 10000, 5000, 0.33
ENVMAP_TEXELS, ENVMAP_EMA, ENVMAP_GRADIENT, ENVMAP_CELLS = 0, 1, 2, 3  # nrs_envmap_what
RAY_AUX_WORDS = 12  # NRS_RAY_AUX_WORDS
EXPOSURE_VALUES, EXPOSURE_M, EXPOSURE_V, EXPOSURE_CELLS, EXPOSURE_GRADIENT = 0, 1, 2, 3, 4  # nrs_exposure_what
EXPOSURE_MAX_IMAGES = 1 << 20  # NRS_EXPOSURE_MAX_IMAGES

# every symbol include/nrs.h declares; tests check the library exports exactly these
EXPORTS = [
    "nrs_last_error", "nrs_abi_version", "nrs_edit_poisson_interpolate", "nrs_edit_download_poisson", "nrs_comm_unique_id", "nrs_comm_create", "nrs_comm_info", "nrs_comm_destroy", "nrs_gather_tiles", "nrs_comm_probe_self_p2p",
    "nrs_ctx_create", "nrs_ctx_destroy", "nrs_ctx_device_info", "nrs_ctx_set_lane_teams", "nrs_ctx_set_ray_handover", "nrs_ctx_ray_handovers",
    "nrs_model_create", "nrs_model_destroy", "nrs_model_n_params", "nrs_model_level_table",
    "nrs_model_set_params", "nrs_model_set_params_device", "nrs_model_set_numerics", "nrs_model_set_cell_cache", "nrs_model_cell_cache_bytes", "nrs_model_set_sparse_cell_cache", "nrs_model_sparse_cell_cache_bytes", "nrs_model_set_density_bitfield", "nrs_model_set_density_grid",
    "nrs_model_get_density_bitfield", "nrs_model_get_march_accelerator", "nrs_model_get_density_grid", "nrs_model_update_density_grid", "nrs_rng_seed",
    "nrs_network_inference", "nrs_network_density", "nrs_hashgrid_encode", "nrs_density_on_grid", "nrs_rgba_on_grid", "nrs_network_input_gradient", "nrs_network_visualize_activation",
    "nrs_poisson_boundary", "nrs_poisson_sample_coords", "nrs_project_selection_pixels", "nrs_upper_cell_idx", "nrs_selection_cells",
    "nrs_edit_create", "nrs_edit_create_affine", "nrs_edit_destroy", "nrs_edit_map_rays", "nrs_edit_map_positions",
    "nrs_edit_set_mvc", "nrs_edit_update_cage", "nrs_edit_update_vertices", "nrs_edit_lut_size", "nrs_edit_download",
    "nrs_render_nerf", "nrs_render_owned_tiles", "nrs_render_tile_pitch", "nrs_detile", "nrs_trace_samples", "nrs_accumulate",
    "nrs_snapshot_open", "nrs_snapshot_close", "nrs_snapshot_model_desc", "nrs_snapshot_params_fp16", "nrs_snapshot_density_grid",
    "nrs_snapshot_camera", "nrs_edits_open", "nrs_edits_close", "nrs_edits_count", "nrs_edits_type", "nrs_edits_cage", "nrs_edits_affine",
    "nrs_tet_lut_build", "nrs_tet_lut_n_idx", "nrs_tet_lut_max_per_cell", "nrs_tet_lut_offsets",
    "nrs_tet_lut_idx", "nrs_tet_lut_bitfield", "nrs_tet_lut_destroy",
    "nrs_mvc_compute", "nrs_mvc_apply", "nrs_tet_local_rotations",
    "nrs_render_nerf_spp", "nrs_accumulate_spp", "nrs_ctx_render_launches",
    "nrs_model_create_ex", "nrs_model_n_params_ex", "nrs_model_n_extra_dims", "nrs_model_set_light_dir", "nrs_network_inference_strided",
    "nrs_snapshot_open_ex", "nrs_snapshot_n_extra_dims",
    "nrs_tonemap", "nrs_accumulate_spp_tonemap", "nrs_tonemap_output_bytes",
    "nrs_render_nerf_spp_views", "nrs_log_space_lerp", "nrs_camera_keyframe_matrix", "nrs_camera_keyframe_from_matrix", "nrs_camera_path_eval",
    "nrs_camera_path_open", "nrs_camera_path_count", "nrs_camera_path_keyframes", "nrs_camera_path_close", "nrs_motion_views",
    "nrs_marching_cubes_res", "nrs_marching_cubes_table", "nrs_mesh_write", "nrs_mesh_from_density", "nrs_mesh_extract", "nrs_mesh_color_inputs",
    "nrs_mesh_counts", "nrs_mesh_device", "nrs_mesh_download", "nrs_mesh_destroy",
    "nrs_selection_create", "nrs_selection_destroy", "nrs_selection_reset", "nrs_selection_grow", "nrs_selection_upscale", "nrs_selection_state",
    "nrs_selection_get_cells", "nrs_selection_get_bitfield", "nrs_selection_set_structuring_elements", "nrs_bitfield_morph", "nrs_bitfield_morph_host",
    "nrs_selection_dilate", "nrs_selection_erode", "nrs_selection_fine_mesh",
    "nrs_network_backward",
    "nrs_training_samples", "nrs_ray_loss",
    "nrs_adam_bias_table", "nrs_exponential_decay_lr", "nrs_optimizer_create", "nrs_optimizer_create_for_model", "nrs_optimizer_destroy", "nrs_optimizer_set_weights",
    "nrs_optimizer_step", "nrs_optimizer_get_state", "nrs_optimizer_set_state", "nrs_optimizer_export_fp16", "nrs_optimizer_step_count", "nrs_optimizer_set_step_count",
    "nrs_optimizer_n_params",
    "nrs_dataset_create", "nrs_dataset_destroy", "nrs_dataset_set_image", "nrs_dataset_set_camera", "nrs_dataset_get_image", "nrs_dataset_rays", "nrs_dataset_mark_untrained", "nrs_rng_advance",
    "nrs_dataset_error_map_reset", "nrs_error_map_resolution", "nrs_dataset_error_map_set", "nrs_dataset_error_map_get", "nrs_dataset_error_map_accumulate",
    "nrs_dataset_error_map_build_cdfs", "nrs_error_map_cdfs_host", "nrs_dataset_rays_ex",
    "nrs_image_metrics", "nrs_dataset_image_metrics", "nrs_image_metrics_host", "nrs_image_metrics_summary_host",
    "nrs_envmap_default_adam_params", "nrs_envmap_create", "nrs_envmap_destroy", "nrs_envmap_resolution", "nrs_envmap_set_texels", "nrs_envmap_get", "nrs_envmap_export",
    "nrs_envmap_background", "nrs_ray_loss_ex", "nrs_envmap_accumulate", "nrs_envmap_step", "nrs_envmap_step_count",
    "nrs_exposure_default_params", "nrs_exposure_create", "nrs_exposure_destroy", "nrs_exposure_n_images", "nrs_exposure_step_count", "nrs_exposure_set", "nrs_exposure_get",
    "nrs_exposure_export", "nrs_exposure_targets", "nrs_exposure_accumulate", "nrs_exposure_step", "nrs_exposure_step_host",
]
SNAPSHOT_ALLOW_LIGHT_DIRS = 1  # NRS_SNAPSHOT_ALLOW_LIGHT_DIRS
SPP_BATCH_MAX = 64  # NRS_SPP_BATCH_MAX
COLOR_LINEAR, COLOR_SRGB, COLOR_VISPOSNEG = 0, 1, 2  # nrs_color_space
TONEMAP_IDENTITY, TONEMAP_ACES, TONEMAP_HABLE, TONEMAP_REINHARD = 0, 1, 2, 3  # nrs_tonemap_curve
TONEMAP_RGBA32F, TONEMAP_RGBA8 = 0, 1  # NRS_TONEMAP_RGBA32F / _RGBA8
SE_CUBE, SE_SPHERE = 0, 1  # NRS_SE_CUBE / _SPHERE (ESEType)
MORPH_DILATE, MORPH_ERODE = 0, 1  # NRS_MORPH_DILATE / _ERODE
MESH_THRESH_DEFAULT = 2.5  # m_mesh.thresh as the reference's Python interface passes it (testbed.h:387)

_lib = None


class NrsError(RuntimeError):
    pass


def load():
    """Load libnrs.so (built in-tree by __graft_entry__.build()).  Fails loudly when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NrsError(
            f"{LIB_PATH} is missing: the HIP extension has not been built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback.")
    # One HIP runtime per process: PyTorch bundles its own libamdhip64.so (SONAME libamdhip64.so.7).  Importing torch
    # first makes the dynamic linker bind libnrs.so's NEEDED libamdhip64.so.7 to that already-loaded copy, so torch
    # tensors and our kernels share a device context (two runtimes in one process cannot both open the GPU).
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    P, U32, I = C.c_void_p, C.c_uint32, C.c_int
    lib.nrs_last_error.restype = C.c_char_p
    lib.nrs_abi_version.restype = I
    lib.nrs_ctx_create.argtypes = [I, C.POINTER(P)]
    lib.nrs_ctx_destroy.argtypes = [P]
    lib.nrs_ctx_destroy.restype = None
    lib.nrs_ctx_device_info.argtypes = [P, C.c_char_p, C.c_size_t, C.POINTER(I), C.POINTER(C.c_size_t)]
    lib.nrs_model_create.argtypes = [P, C.POINTER(ModelDesc), C.POINTER(P)]
    lib.nrs_ctx_set_lane_teams.argtypes = [P, C.c_int]
    lib.nrs_ctx_set_ray_handover.argtypes = [P, C.c_int]
    lib.nrs_ctx_ray_handovers.argtypes = [P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.nrs_model_destroy.argtypes = [P]
    lib.nrs_model_destroy.restype = None
    lib.nrs_model_n_params.argtypes = [C.POINTER(ModelDesc)]
    lib.nrs_model_n_params.restype = C.c_size_t
    lib.nrs_model_level_table.argtypes = [C.POINTER(ModelDesc), P, P, P, P, P]
    lib.nrs_model_set_params.argtypes = [P, P, C.c_size_t]
    lib.nrs_project_selection_pixels.argtypes = [P, P, C.POINTER(RenderParams), P, C.c_uint32, C.c_float, P, P, P]
    lib.nrs_poisson_boundary.argtypes = [P, P, C.c_uint32, C.c_uint32, C.c_uint32, P, C.c_int, P, P]
    lib.nrs_poisson_sample_coords.argtypes = [P, C.c_uint32, C.c_uint32, C.c_uint32, P, P, P, P]
    lib.nrs_poisson_sample_coords.restype = None
    lib.nrs_upper_cell_idx.argtypes = [C.c_uint32, C.c_uint32]
    lib.nrs_upper_cell_idx.restype = C.c_uint32
    lib.nrs_selection_cells.argtypes = [P, P, P, C.c_uint32, C.c_int, P, P, P, P]
    lib.nrs_model_set_cell_cache.argtypes = [P, C.c_size_t]
    lib.nrs_model_cell_cache_bytes.argtypes = [P, P]
    lib.nrs_model_cell_cache_bytes.restype = C.c_size_t
    lib.nrs_model_set_numerics.argtypes = [P, C.c_uint32, C.c_uint32]
    lib.nrs_model_set_params_device.argtypes = [P, P, C.c_size_t, P]
    lib.nrs_edit_poisson_interpolate.argtypes = [P, P, P, C.c_uint32, P, P, P, P, C.c_float]
    lib.nrs_edit_download_poisson.argtypes = [P, P, P, P]
    lib.nrs_comm_unique_id.argtypes = [P]
    lib.nrs_comm_create.argtypes = [C.c_int, C.c_int, C.c_int, P, P]
    lib.nrs_comm_info.argtypes = [P, P, P, P, P, C.c_size_t]
    lib.nrs_comm_destroy.argtypes = [P]
    lib.nrs_comm_destroy.restype = None
    lib.nrs_gather_tiles.argtypes = [P, P, C.c_int, P, C.c_uint32, P, P, P, P, P]
    lib.nrs_comm_probe_self_p2p.argtypes = [P, P, P, C.c_size_t, C.c_int, P]
    lib.nrs_model_set_sparse_cell_cache.argtypes = [P, P, C.c_size_t]
    lib.nrs_model_sparse_cell_cache_bytes.argtypes = [P, P, P]
    lib.nrs_model_sparse_cell_cache_bytes.restype = C.c_size_t
    lib.nrs_model_set_density_bitfield.argtypes = [P, P, C.c_size_t]
    lib.nrs_model_set_density_grid.argtypes = [P, P, C.c_size_t]
    lib.nrs_model_get_density_bitfield.argtypes = [P, P, C.c_size_t]
    lib.nrs_model_get_density_grid.argtypes = [P, P, C.c_size_t]
    lib.nrs_model_get_march_accelerator.argtypes = [P, I, P, P]
    lib.nrs_model_update_density_grid.argtypes = [P, C.POINTER(P), I, C.POINTER(GridUpdate), P]
    lib.nrs_rng_seed.argtypes = [C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.nrs_rng_seed.restype = None
    lib.nrs_network_inference.argtypes = [P, P, U32, P, P, U32, I]
    lib.nrs_network_density.argtypes = [P, P, U32, P, U32, P, U32, I]
    lib.nrs_hashgrid_encode.argtypes = [P, P, U32, P, U32, P]
    lib.nrs_network_input_gradient.argtypes = [P, P, U32, P, U32, P]
    lib.nrs_network_visualize_activation.argtypes = [P, P, U32, U32, U32, P, P]
    if hasattr(lib, "nrs_network_backward"):  # (an A/B build of the parent tree through NRS_LIB_PATH has none: tools/network_backward_probe.py --parent-lib)
        lib.nrs_network_backward.argtypes = [P, P, U32, P, U32, P, U32, I, P, C.c_size_t, I, P]
    if hasattr(lib, "nrs_ray_loss"):  # (detected by symbol, like nrs_network_backward)
        lib.nrs_training_samples.argtypes = [P, P, U32, P, P, C.c_float, U32, P, U32, P, P, P]
        lib.nrs_ray_loss.argtypes = [P, P, C.POINTER(RayLossParams), U32, P, P, U32, P, U32, P, U32, I, P, P, P, P, P, P, U32, I, P, P]
    if hasattr(lib, "nrs_optimizer_step"):  # (detected by symbol, like nrs_network_backward)
        lib.nrs_adam_bias_table.argtypes = [C.c_float, C.c_float, P, U32, C.POINTER(U32)]
        lib.nrs_exponential_decay_lr.argtypes = [C.c_float, U32, U32, C.c_float, U32]
        lib.nrs_exponential_decay_lr.restype = C.c_float
        lib.nrs_optimizer_create.argtypes = [P, C.c_size_t, C.c_size_t, C.POINTER(AdamParams), C.POINTER(P)]
        lib.nrs_optimizer_create_for_model.argtypes = [P, C.POINTER(AdamParams), C.POINTER(P)]
        lib.nrs_optimizer_destroy.argtypes = [P]
        lib.nrs_optimizer_destroy.restype = None
        lib.nrs_optimizer_set_weights.argtypes = [P, P, I, P]
        lib.nrs_optimizer_step.argtypes = [P, P, P, C.c_float, C.c_float, I]
        lib.nrs_optimizer_get_state.argtypes = [P, I, P, C.c_size_t]
        lib.nrs_optimizer_set_state.argtypes = [P, I, P, C.c_size_t]
        lib.nrs_optimizer_export_fp16.argtypes = [P, I, P, P]
        lib.nrs_optimizer_step_count.argtypes = [P]
        lib.nrs_optimizer_step_count.restype = U32
        lib.nrs_optimizer_set_step_count.argtypes = [P, U32]
        lib.nrs_optimizer_n_params.argtypes = [P, C.POINTER(C.c_size_t)]
        lib.nrs_optimizer_n_params.restype = C.c_size_t
    if hasattr(lib, "nrs_dataset_rays"):  # (detected by symbol, like nrs_network_backward)
        lib.nrs_dataset_create.argtypes = [P, U32, U32, U32, C.POINTER(P)]
        lib.nrs_dataset_destroy.argtypes = [P]
        lib.nrs_dataset_destroy.restype = None
        lib.nrs_dataset_set_image.argtypes = [P, U32, I, P, I, U32, U32, P]
        lib.nrs_dataset_set_camera.argtypes = [P, U32, C.POINTER(TrainingCamera)]
        lib.nrs_dataset_get_image.argtypes = [P, U32, P]
        lib.nrs_dataset_rays.argtypes = [P, P, C.POINTER(DatasetRaysParams), U32, P, P, P, P, P]
        lib.nrs_dataset_mark_untrained.argtypes = [P, P, I, P]
        lib.nrs_rng_advance.argtypes = [C.POINTER(C.c_uint64), C.c_uint64, C.c_uint64]
        lib.nrs_rng_advance.restype = None
    if hasattr(lib, "nrs_dataset_rays_ex"):  # the training error map (detected by symbol)
        lib.nrs_dataset_error_map_reset.argtypes = [P, U32, U32, P]
        lib.nrs_error_map_resolution.argtypes = [U32, U32, U32, U32]
        lib.nrs_error_map_resolution.restype = U32
        lib.nrs_dataset_error_map_set.argtypes = [P, U32, U32, P]
        lib.nrs_dataset_error_map_get.argtypes = [P, I, P, C.POINTER(C.c_size_t)]
        lib.nrs_dataset_error_map_accumulate.argtypes = [P, P, U32, P, P, P, P, P, P, P]
        lib.nrs_dataset_error_map_build_cdfs.argtypes = [P, P]
        lib.nrs_error_map_cdfs_host.argtypes = [U32, U32, U32, P, P, P, P, P]
        lib.nrs_dataset_rays_ex.argtypes = [P, P, C.POINTER(DatasetRaysExParams), U32, P, P, P, P, P, P, P]
    if hasattr(lib, "nrs_image_metrics"):  # image metrics (detected by symbol)
        lib.nrs_image_metrics.argtypes = [P, P, U32, U32, P, P, C.POINTER(ImageMetricsParams), P, P, P]
        lib.nrs_dataset_image_metrics.argtypes = [P, U32, P, P, C.POINTER(ImageMetricsParams), P, P, P]
        lib.nrs_image_metrics_host.argtypes = [U32, U32, P, P, C.POINTER(ImageMetricsParams), P, P, P]
        lib.nrs_image_metrics_summary_host.argtypes = [P, U32, C.POINTER(MetricsSummary)]
    if hasattr(lib, "nrs_envmap_create"):  # the trainable environment map (detected by symbol)
        lib.nrs_envmap_default_adam_params.argtypes = [C.POINTER(AdamParams)]
        lib.nrs_envmap_default_adam_params.restype = None
        lib.nrs_envmap_create.argtypes = [P, U32, U32, C.POINTER(AdamParams), C.POINTER(P)]
        lib.nrs_envmap_destroy.argtypes = [P]
        lib.nrs_envmap_destroy.restype = None
        lib.nrs_envmap_resolution.argtypes = [P, C.POINTER(U32), C.POINTER(U32)]
        lib.nrs_envmap_set_texels.argtypes = [P, P, I, P]
        lib.nrs_envmap_get.argtypes = [P, I, P, C.c_size_t]
        lib.nrs_envmap_export.argtypes = [P, I, P, P]
        lib.nrs_envmap_background.argtypes = [P, P, U32, P, P, P, P, C.POINTER(C.c_float * 3), P, P]
        lib.nrs_ray_loss_ex.argtypes = [P, P, C.POINTER(RayLossParams), U32, P, P, U32, P, U32, P, U32, I, P, P, P, P, P, P, U32, I, P, P, P, P]
        lib.nrs_envmap_accumulate.argtypes = [P, P, C.POINTER(EnvmapAccumulateParams), U32, P, P, P, P, P]
        lib.nrs_envmap_step.argtypes = [P, P, C.c_float, C.c_float]
        lib.nrs_envmap_step_count.argtypes = [P]
        lib.nrs_envmap_step_count.restype = U32
    if hasattr(lib, "nrs_exposure_create"):  # per-image exposure (detected by symbol)
        lib.nrs_exposure_default_params.argtypes = [C.POINTER(ExposureParams)]
        lib.nrs_exposure_default_params.restype = None
        lib.nrs_exposure_create.argtypes = [P, U32, C.POINTER(ExposureParams), C.POINTER(P)]
        lib.nrs_exposure_destroy.argtypes = [P]
        lib.nrs_exposure_destroy.restype = None
        lib.nrs_exposure_n_images.argtypes = [P]
        lib.nrs_exposure_n_images.restype = U32
        lib.nrs_exposure_step_count.argtypes = [P]
        lib.nrs_exposure_step_count.restype = U32
        lib.nrs_exposure_set.argtypes = [P, P]
        lib.nrs_exposure_get.argtypes = [P, I, P, C.c_size_t]
        lib.nrs_exposure_export.argtypes = [P, P, P]
        lib.nrs_exposure_targets.argtypes = [P, P, U32, P, P, P, P, P, P]
        lib.nrs_exposure_accumulate.argtypes = [P, P, C.POINTER(ExposureAccumulateParams), U32, P, P, P, P, P, P]
        lib.nrs_exposure_step.argtypes = [P, P, C.c_float, C.c_float]
        lib.nrs_exposure_step_host.argtypes = [U32, C.POINTER(ExposureParams), C.c_float, C.c_float, P, P, P, P, C.POINTER(U32)]
    lib.nrs_density_on_grid.argtypes = [P, P, C.POINTER(U32 * 3), C.POINTER(C.c_float * 3), C.POINTER(C.c_float * 3), I, P]
    lib.nrs_rgba_on_grid.argtypes = [P, P, C.POINTER(U32 * 3), C.POINTER(C.c_float * 3), C.POINTER(C.c_float * 3), C.POINTER(C.c_float * 3), P]
    lib.nrs_edit_create.argtypes = [P, C.POINTER(ModelDesc), C.POINTER(TetMesh), C.POINTER(P)]
    lib.nrs_edit_create_affine.argtypes = [P, C.POINTER(ModelDesc), C.POINTER(AffineDuplicationOp), C.POINTER(P)]
    lib.nrs_edits_affine.argtypes = [P, U32, C.POINTER(AffineDuplicationOp)]
    lib.nrs_edit_destroy.argtypes = [P]
    lib.nrs_edit_destroy.restype = None
    lib.nrs_edit_map_rays.argtypes = [P, P, U32, P, P]
    lib.nrs_edit_map_positions.argtypes = [P, P, U32, P, U32, P]
    lib.nrs_edit_set_mvc.argtypes = [P, P, U32]
    lib.nrs_edit_update_cage.argtypes = [P, P, P, U32]
    lib.nrs_edit_update_vertices.argtypes = [P, P, P, U32]
    lib.nrs_edit_lut_size.argtypes = [P, C.POINTER(U32), C.POINTER(U32)]
    lib.nrs_edit_download.argtypes = [P, P, P, P, P, P, P]
    lib.nrs_render_nerf.argtypes = [P, C.POINTER(RenderParams), C.POINTER(P), I, P, P, P, P, C.POINTER(RenderStats)]
    lib.nrs_render_owned_tiles.argtypes = [C.POINTER(RenderParams)]
    lib.nrs_render_owned_tiles.restype = U32
    lib.nrs_render_tile_pitch.argtypes = [C.POINTER(RenderParams)]
    lib.nrs_render_tile_pitch.restype = U32
    lib.nrs_detile.argtypes = [P, P, C.POINTER(RenderParams), U32, U32, P, U32, C.c_size_t, P]
    lib.nrs_trace_samples.argtypes = [P, C.POINTER(RenderParams), P, U32, P, U32, P, P, P]
    lib.nrs_accumulate.argtypes = [P, P, U32, U32, P, P, U32, U32]
    # several samples per pixel in one launch (appended exports: a library without them predates the feature -- callers may test with hasattr)
    if hasattr(lib, "nrs_render_nerf_spp"):  # (an A/B build of an older tree through NRS_LIB_PATH has none of the three)
        lib.nrs_render_nerf_spp.argtypes = [P, C.POINTER(RenderParams), C.POINTER(P), I, U32, P, P, P, C.c_size_t, P, C.POINTER(RenderStats)]
        lib.nrs_accumulate_spp.argtypes = [P, P, U32, U32, P, C.c_size_t, U32, P, U32, U32]
        lib.nrs_ctx_render_launches.argtypes = [P, C.POINTER(C.c_uint64), C.POINTER(U32)]
    # networks trained with light directions (appended exports, detected by symbol like the spp batch)
    if hasattr(lib, "nrs_model_create_ex"):
        lib.nrs_model_create_ex.argtypes = [P, C.POINTER(ModelDesc), U32, C.POINTER(P)]
        lib.nrs_model_n_params_ex.argtypes = [C.POINTER(ModelDesc), U32]
        lib.nrs_model_n_params_ex.restype = C.c_size_t
        lib.nrs_model_n_extra_dims.argtypes = [P]
        lib.nrs_model_set_light_dir.argtypes = [P, C.POINTER(C.c_float * 3)]
        lib.nrs_network_inference_strided.argtypes = [P, P, U32, P, U32, P, U32, I]
        lib.nrs_snapshot_open_ex.argtypes = [C.c_char_p, U32, C.POINTER(P)]
        lib.nrs_snapshot_n_extra_dims.argtypes = [P]
        lib.nrs_snapshot_n_extra_dims.restype = U32
    # the display step after accumulate (appended exports, detected by symbol like the spp batch)
    if hasattr(lib, "nrs_tonemap"):
        lib.nrs_tonemap.argtypes = [P, P, U32, U32, P, C.POINTER(TonemapParams), P]
        lib.nrs_accumulate_spp_tonemap.argtypes = [P, P, U32, U32, P, C.c_size_t, U32, P, U32, C.POINTER(TonemapParams), P]
        lib.nrs_tonemap_output_bytes.argtypes = [U32, U32, U32]
        lib.nrs_tonemap_output_bytes.restype = C.c_size_t
    # a view per sample and the cameras of render_to_cpu's loop (appended exports, detected by symbol like the spp batch)
    if hasattr(lib, "nrs_render_nerf_spp_views"):
        F12 = C.POINTER(C.c_float * 12)
        lib.nrs_render_nerf_spp_views.argtypes = [P, C.POINTER(RenderParams), C.POINTER(P), I, U32, P, P, P, P, C.c_size_t, P, C.POINTER(RenderStats)]
        lib.nrs_log_space_lerp.argtypes = [F12, F12, C.c_float, F12]
        lib.nrs_camera_keyframe_matrix.argtypes = [C.POINTER(CameraKeyframe), F12]
        lib.nrs_camera_keyframe_from_matrix.argtypes = [F12, C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(CameraKeyframe)]
        lib.nrs_camera_path_eval.argtypes = [P, U32, C.c_float, C.POINTER(CameraKeyframe)]
        lib.nrs_camera_path_open.argtypes = [C.c_char_p, C.POINTER(P)]
        lib.nrs_camera_path_count.argtypes = [P]
        lib.nrs_camera_path_count.restype = U32
        lib.nrs_camera_path_keyframes.argtypes = [P, P, U32]
        lib.nrs_camera_path_close.argtypes = [P]
        lib.nrs_camera_path_close.restype = None
        lib.nrs_motion_views.argtypes = [F12, F12, C.c_float, U32, U32, U32, C.POINTER(C.c_int32 * 2), I, P, U32, C.c_float, C.c_float, C.POINTER(SampleView), P]
    # mesh extraction (appended exports, detected by symbol like the spp batch)
    if hasattr(lib, "nrs_mesh_from_density"):
        F3, U3 = C.POINTER(C.c_float * 3), C.POINTER(U32 * 3)
        lib.nrs_marching_cubes_res.argtypes = [U32, F3, F3, U3]
        lib.nrs_marching_cubes_table.argtypes = [P, C.POINTER(U32)]
        lib.nrs_mesh_write.argtypes = [C.c_char_p, U32, P, P, P, U32, P, C.c_float, F3]
        lib.nrs_mesh_from_density.argtypes = [P, P, U3, F3, F3, C.c_float, P, C.POINTER(P)]
        lib.nrs_mesh_extract.argtypes = [P, P, U3, F3, F3, C.c_float, I, I, C.POINTER(P)]
        lib.nrs_mesh_color_inputs.argtypes = [P, P, P, P]
        lib.nrs_mesh_counts.argtypes = [P, C.POINTER(U32), C.POINTER(U32), C.POINTER(U32)]
        lib.nrs_mesh_device.argtypes = [P, C.POINTER(P), C.POINTER(P), C.POINTER(P), C.POINTER(P), C.POINTER(P)]
        lib.nrs_mesh_download.argtypes = [P, P, P, P, P, P]
        lib.nrs_mesh_destroy.argtypes = [P]
        lib.nrs_mesh_destroy.restype = None
    # selection tool (appended exports, detected by symbol)
    if hasattr(lib, "nrs_selection_create"):
        PU32 = C.POINTER(U32)
        lib.nrs_selection_create.argtypes = [P, C.c_size_t, U32, C.POINTER(P)]
        lib.nrs_selection_destroy.argtypes = [P]
        lib.nrs_selection_destroy.restype = None
        lib.nrs_selection_reset.argtypes = [P, P, U32, U32]
        lib.nrs_selection_grow.argtypes = [P, C.c_float, U32, U32, PU32]
        lib.nrs_selection_upscale.argtypes = [P]
        lib.nrs_selection_state.argtypes = [P, PU32, PU32, PU32, C.POINTER(I)]
        lib.nrs_selection_get_cells.argtypes = [P, P, P]
        lib.nrs_selection_get_bitfield.argtypes = [P, P]
        lib.nrs_selection_set_structuring_elements.argtypes = [P, I, I, I, I]
        lib.nrs_bitfield_morph.argtypes = [P, P, P, U32, I, I, I, P]
        lib.nrs_bitfield_morph_host.argtypes = [P, U32, I, I, I, P]
        lib.nrs_selection_dilate.argtypes = [P, P, P]
        lib.nrs_selection_erode.argtypes = [P, P, P]
        lib.nrs_selection_fine_mesh.argtypes = [P, P, P, I, C.POINTER(P)]
    lib.nrs_snapshot_open.argtypes = [C.c_char_p, C.POINTER(P)]
    lib.nrs_snapshot_close.argtypes = [P]
    lib.nrs_snapshot_close.restype = None
    lib.nrs_snapshot_model_desc.argtypes = [P, C.POINTER(ModelDesc), C.POINTER(U32)]
    lib.nrs_snapshot_params_fp16.argtypes = [P, C.POINTER(C.c_size_t)]
    lib.nrs_snapshot_params_fp16.restype = P
    lib.nrs_snapshot_density_grid.argtypes = [P, C.POINTER(C.c_size_t)]
    lib.nrs_snapshot_density_grid.restype = P
    lib.nrs_snapshot_camera.argtypes = [P, P]
    lib.nrs_edits_open.argtypes = [C.c_char_p, C.POINTER(P)]
    lib.nrs_edits_close.argtypes = [P]
    lib.nrs_edits_close.restype = None
    lib.nrs_edits_count.argtypes = [P]
    lib.nrs_edits_count.restype = U32
    lib.nrs_edits_type.argtypes = [P, U32]
    lib.nrs_edits_type.restype = C.c_char_p
    lib.nrs_edits_cage.argtypes = [P, U32, C.POINTER(TetMesh), C.POINTER(P), C.POINTER(P), C.POINTER(P), C.POINTER(P), C.POINTER(U32), C.POINTER(U32)]
    lib.nrs_tet_lut_build.argtypes = [P, U32, P, U32, I, C.POINTER(P)]
    for name in ("nrs_tet_lut_n_idx", "nrs_tet_lut_max_per_cell"):
        getattr(lib, name).argtypes = [P]
        getattr(lib, name).restype = U32
    for name in ("nrs_tet_lut_offsets", "nrs_tet_lut_idx", "nrs_tet_lut_bitfield"):
        getattr(lib, name).argtypes = [P]
        getattr(lib, name).restype = P
    lib.nrs_tet_lut_destroy.argtypes = [P]
    lib.nrs_tet_lut_destroy.restype = None
    lib.nrs_mvc_compute.argtypes = [P, U32, P, U32, P, U32, P, P]
    lib.nrs_mvc_apply.argtypes = [P, P, U32, U32, P]
    lib.nrs_tet_local_rotations.argtypes = [P, P, P, U32, P]
    _lib = lib
    return lib


def check(status):
    if status != NRS_OK:
        raise NrsError(f"nrs error {status}: {load().nrs_last_error().decode()}")
