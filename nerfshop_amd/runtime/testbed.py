"""The slice of ngp::Testbed the render path reads (nrs_api_render.cpp, nrs_camera.cpp and the Testbed-level calls of the other subsystems)."""
import ctypes as C
import os

import numpy as np
import torch

from .. import _abi
from .._abi import NrsError, RenderParams, RenderStats, check
from ._base import _device, _float3, _ptr, _require_cuda, _stream_handle, _uint3
from .edits import _operator_handles
from .mesh import Mesh
from .network import NerfNetwork, rng_seed
from .render_buffer import RenderBuffer
from .selection import GrowingSelection


def set_camera_extras(p, render_distortion=None, distortion_map=None, envmap=None):
    """Camera model and background of an nrs_render_params (init_rays_from_camera's arguments, testbed_nerf.cu:3078-3100): lens distortion (mode, 7 params),
    the distortion map [H, W, 2] and the environment map [H, W, 4] as float32 CUDA tensors (the struct keeps raw device pointers: keep the tensors alive)."""
    if render_distortion is not None:
        p.distortion_mode = int(render_distortion[0])
        p.distortion_params[:] = [float(v) for v in render_distortion[1]]
    if distortion_map is not None:
        _require_cuda(distortion_map, torch.float32, "distortion_map")
        p.d_distortion_map = distortion_map.data_ptr()
        p.distortion_resolution[:] = (distortion_map.shape[1], distortion_map.shape[0])
    if envmap is not None:
        _require_cuda(envmap, torch.float32, "envmap")
        p.d_envmap = envmap.data_ptr()
        p.envmap_resolution[:] = (envmap.shape[1], envmap.shape[0])
    return p


class Testbed:
    """The slice of ngp::Testbed the render path reads: network, occupancy, edit operators and the render knobs."""

    def __init__(self, ctx, desc, aabb_scale=1, n_extra_dims=0, network=None):
        """network: a NerfNetwork this testbed renders instead of making its own (Trainer.evaluate: the trainer's live network)."""
        self.ctx, self.lib, self.desc = ctx, ctx.lib, desc
        self.nerf_network = network if network is not None else NerfNetwork(ctx, desc, n_extra_dims=n_extra_dims)
        self.edit_operators = []          # NerfTracer::m_edit_operators, applied last-to-first
        self.enable_edits = True          # m_enable_edits
        self.snap_to_pixel_centers = True
        self.rendering_min_transmittance = 0.01
        self.cone_angle_constant = 0.0 if aabb_scale <= 1 else 1.0 / 256.0
        self.render_mode = _abi.RENDER_SHADE
        self.linear_colors = False
        self.show_accel = -1              # m_nerf.show_accel
        self.dof = 0.0                    # m_dof
        self.slice_plane_z, self.scale = 0.0, 1.0   # m_slice_plane_z, m_scale
        self.dataset_scale = 1.0          # m_nerf.training.dataset.scale
        self.render_distortion = (0, (0.0,) * 7)   # m_nerf.render_distortion (mode, params) when render_with_camera_distortion
        self.distortion_map = None        # m_distortion.map: float32 CUDA tensor [H, W, 2] or None
        self.envmap = None                # m_envmap.envmap: float32 CUDA tensor [H, W, 4] or None
        self.glow_mode, self.glow_y_cutoff = 0, 0.0   # m_nerf.m_glow_mode / m_glow_y_cutoff
        mn, mx = list(desc.aabb_min), list(desc.aabb_max)
        self.render_aabb = (mn, mx)       # m_render_aabb
        self.last_stats = None
        self.m_camera = None              # m_camera: 3x4 column-major [12]; set by set_camera_from_time / render_to_cpu
        self.m_smoothed_camera = None     # m_smoothed_camera: the camera the last frame ended on
        self.camera_smoothing = False     # m_camera_smoothing
        self.fov, self.fov_axis = 50.625, 1   # fov() in degrees (set_camera_from_time sets it), m_fov_axis
        self.camera_path = []             # m_camera_path.m_keyframes: a list of _abi.CameraKeyframe
        self._windowless = None           # m_windowless_render_surface: the RenderBuffer of render_to_cpu
        self._evaluate_surface = None     # the RenderBuffer of evaluate
        self.mesh = None                  # m_mesh: the Mesh of the last marching_cubes

    def add_edit_operator(self, op):
        self.edit_operators.append(op)

    def training_samples(self, rays, jitter=None, max_samples=1 << 18, cone_angle_constant=None, stream=None):
        """The network inputs of a batch of training rays (NerfNetwork.training_samples) with this testbed's cone angle: coords, numsteps, ray_indices, counters."""
        cone = self.cone_angle_constant if cone_angle_constant is None else cone_angle_constant
        return self.nerf_network.training_samples(stream, rays, jitter, cone, max_samples)

    def make_params(self, render_buffer, focal_length, camera_matrix0, camera_matrix1, rolling_shutter, screen_center, apply_operators):
        p = RenderParams()
        p.resolution[:] = render_buffer.in_resolution()
        p.focal_length[:] = list(focal_length)
        p.camera_matrix0[:] = [float(v) for v in np.asarray(camera_matrix0, np.float32).reshape(-1)]
        p.camera_matrix1[:] = [float(v) for v in np.asarray(camera_matrix1, np.float32).reshape(-1)]
        p.rolling_shutter[:] = list(rolling_shutter)
        p.screen_center[:] = list(screen_center)
        p.render_aabb_min[:] = self.render_aabb[0]
        p.render_aabb_max[:] = self.render_aabb[1]
        p.spp_index = render_buffer.spp()
        p.snap_to_pixel_centers = 1 if self.snap_to_pixel_centers else 0
        p.min_transmittance = self.rendering_min_transmittance
        p.cone_angle_constant = self.cone_angle_constant
        p.render_mode = self.render_mode
        p.linear_colors = 1 if self.linear_colors else 0
        p.apply_operators = 1 if apply_operators else 0
        p.min_mip = self.show_accel if self.show_accel >= 0 else 0
        p.show_accel = 1 if self.show_accel >= 0 else 0
        p.dof = self.dof
        p.slice_plane_z = self.slice_plane_z + self.scale  # testbed_nerf.cu:3067
        p.depth_scale = 1.0 / self.dataset_scale           # :3113
        p.glow_mode, p.glow_y_cutoff = self.glow_mode, self.glow_y_cutoff
        set_camera_extras(p, self.render_distortion, self.distortion_map, self.envmap)
        return p

    def render_nerf(self, network, render_buffer, max_res, focal_length, camera_matrix0, camera_matrix1, rolling_shutter, screen_center,
                    apply_operators, stream=None, want_stats=False):
        """Testbed::render_nerf(network, render_buffer, max_res, focal_length, camera_matrix0, camera_matrix1, rolling_shutter,
        screen_center, apply_operators, stream).  The frame buffer must have been cleared by the caller (render_frame does)."""
        p = self.make_params(render_buffer, focal_length, camera_matrix0, camera_matrix1, rolling_shutter, screen_center,
                             apply_operators and self.enable_edits)
        return self.render_with_params(network, p, render_buffer.frame_buffer(), render_buffer.depth_buffer(), render_buffer.steps_buffer(),
                                       stream, want_stats)

    def render_with_params(self, network, p, frame, depth, steps=None, stream=None, want_stats=False):
        _require_cuda(frame, torch.float32, "frame_buffer")
        _require_cuda(depth, torch.float32, "depth_buffer")
        return self._render(self.lib.nrs_render_nerf, network, p, (), frame, depth, steps, (), stream, want_stats)

    def _render(self, entry, network, p, batch, frames, depths, steps, slab_stride, stream, want_stats):
        """The call the three render entry points share: (network, params, operators, n_operators, *batch, frames, depths, steps, *slab_stride, stream, stats).
        The operator array, the statistics and last_stats are made here."""
        arr, n = _operator_handles(self.edit_operators)
        stats = RenderStats() if want_stats else None
        check(entry(network.h, C.byref(p), arr, n, *batch, frames.data_ptr(), depths.data_ptr(), _ptr(steps), *slab_stride, _stream_handle(stream),
                    C.byref(stats) if stats is not None else None))
        self.last_stats = stats
        return stats

    @staticmethod
    def _slab_stride(frames, slab_stride_pixels):
        """The pixels between two slabs of frames [K, H, W, 4]: what was given, or the elements of frames[0] / 4"""
        if slab_stride_pixels is None:
            slab_stride_pixels = frames[0].numel() // 4 if frames.dim() > 1 and frames.shape[0] else 0
        return int(slab_stride_pixels)

    def render_nerf_spp(self, network, render_buffer, spp_count, focal_length, camera_matrix0, camera_matrix1, rolling_shutter, screen_center,
                        apply_operators, stream=None, want_stats=False):
        """Samples spp() .. spp() + spp_count - 1 of the view in ONE launch (what the spp loop of the reference's render_to_cpu does in spp_count launches): returns
        (frames [K, H, W, 4], depths [K, H, W], steps or None, stats).  Follow with render_buffer.accumulate_spp(ctx, frames), which advances spp() by K."""
        p = self.make_params(render_buffer, focal_length, camera_matrix0, camera_matrix1, rolling_shutter, screen_center,
                             apply_operators and self.enable_edits)
        frames, depths, steps = render_buffer.spp_slabs(spp_count)
        stats = self.render_spp_with_params(network, p, spp_count, frames, depths, steps, None, stream, want_stats)
        return frames, depths, steps, stats

    def render_spp_with_params(self, network, p, spp_count, frames, depths, steps=None, slab_stride_pixels=None, stream=None, want_stats=False):
        """nrs_render_nerf_spp: slab k of frames / depths / steps (slab_stride_pixels apart; default: the elements of frames[0] / 4) receives sample p.spp_index + k."""
        _require_cuda(frames, torch.float32, "frames")
        _require_cuda(depths, torch.float32, "depths")
        return self._render(self.lib.nrs_render_nerf_spp, network, p, (int(spp_count),), frames, depths, steps,
                            (self._slab_stride(frames, slab_stride_pixels),), stream, want_stats)

    def render_spp_with_views(self, network, p, views, frames, depths, steps=None, slab_stride_pixels=None, stream=None, want_stats=False, spp_count=None):
        """nrs_render_nerf_spp_views: slab k receives sample p.spp_index + k rendered with views[k] (a ctypes array of _abi.SampleView, or a list of them) in place of
        p's cameras, focal length, dof and slice_plane_z.  One launch for the whole batch.  views = None is nrs_render_nerf_spp of `spp_count` samples; spp_count
        defaults to len(views)."""
        _require_cuda(frames, torch.float32, "frames")
        _require_cuda(depths, torch.float32, "depths")
        if views is not None and not isinstance(views, C.Array):
            views = (_abi.SampleView * max(len(views), 1))(*views)
        if spp_count is None:
            spp_count = len(views)
        return self._render(self.lib.nrs_render_nerf_spp_views, network, p, (int(spp_count), C.cast(views, C.c_void_p) if views is not None else None),
                            frames, depths, steps, (self._slab_stride(frames, slab_stride_pixels),), stream, want_stats)

    # ---- the camera path (CameraPath, Testbed::set_camera_from_time / apply_camera_smoothing) ----
    def load_camera_path(self, path):
        """Testbed::load_camera_path -> CameraPath::load (src/camera_path.cu:114-136): the keyframes of a file CameraPath::save wrote; returns their number"""
        h = C.c_void_p()
        check(self.lib.nrs_camera_path_open(os.fsencode(path), C.byref(h)))
        try:
            n = self.lib.nrs_camera_path_count(h)
            keys = (_abi.CameraKeyframe * max(n, 1))()
            check(self.lib.nrs_camera_path_keyframes(h, C.cast(keys, C.c_void_p), n))
        finally:
            self.lib.nrs_camera_path_close(h)
        self.camera_path = [keys[i] for i in range(n)]
        return n

    def _path_array(self):
        n = len(self.camera_path)
        return (_abi.CameraKeyframe * max(n, 1))(*self.camera_path), n

    def set_camera_from_time(self, t):
        """Testbed::set_camera_from_time (src/testbed.cu:2099-2111): m_camera, slice / scale, fov and dof from the path's keyframe at t; nothing without a path"""
        keys, n = self._path_array()
        if n == 0:
            return
        k = _abi.CameraKeyframe()
        check(self.lib.nrs_camera_path_eval(C.cast(keys, C.c_void_p), n, float(t), C.byref(k)))
        m = (C.c_float * 12)()
        check(self.lib.nrs_camera_keyframe_matrix(C.byref(k), C.byref(m)))
        self.m_camera = list(m)
        self.slice_plane_z, self.scale, self.fov, self.dof = k.slice, k.scale, k.fov, k.dof

    def log_space_lerp(self, begin, end, t):
        a, b, out = (C.c_float * 12)(*[float(v) for v in begin]), (C.c_float * 12)(*[float(v) for v in end]), (C.c_float * 12)()
        check(self.lib.nrs_log_space_lerp(C.byref(a), C.byref(b), float(t), C.byref(out)))
        return list(out)

    def apply_camera_smoothing(self, elapsed_ms):
        """Testbed::apply_camera_smoothing (src/testbed.cu:2086-2093)"""
        if self.camera_smoothing and self.m_smoothed_camera is not None:
            decay = float(np.float32(0.02) ** np.float32(elapsed_ms / 1000.0))
            self.m_smoothed_camera = self.log_space_lerp(self.m_smoothed_camera, self.m_camera, float(np.float32(1.0) - np.float32(decay)))
        else:
            self.m_smoothed_camera = list(self.m_camera)

    def motion_views(self, start, end, shutter_fraction, spp_count, first_sample, spp_total, resolution, start_time, end_time, base_view):
        """nrs_motion_views over this testbed's camera path -> a ctypes array of spp_count _abi.SampleView"""
        keys, n = self._path_array()
        a, b = (C.c_float * 12)(*[float(v) for v in start]), (C.c_float * 12)(*[float(v) for v in end])
        res = (C.c_int32 * 2)(int(resolution[0]), int(resolution[1]))
        out = (_abi.SampleView * int(spp_count))()
        check(self.lib.nrs_motion_views(C.byref(a), C.byref(b), float(shutter_fraction), int(spp_count), int(first_sample), int(spp_total), C.byref(res), int(self.fov_axis),
                                        C.cast(keys, C.c_void_p) if n else None, n, float(start_time), float(end_time), C.byref(base_view), C.cast(out, C.c_void_p)))
        return out

    def render_to_cpu(self, network, width, height, spp, linear, focal_length, camera_matrix0, camera_matrix1=None, rolling_shutter=(0.0, 0.0, 0.0, 0.0),
                      screen_center=(0.5, 0.5), exposure=0.0, background=(0.0, 0.0, 0.0, 0.0), fmt="rgba32f", tonemap_curve=0, color_space=0, apply_operators=True,
                      stream=None, start_time=-1.0, end_time=-1.0, fps=30.0, shutter_fraction=1.0, motion_blur=None):
        """Testbed::render_to_cpu(width, height, spp, linear, start_time, end_time, fps, shutter_fraction) (src/python_api.cu:129-175): the accumulation is reset, `spp`
        samples are rendered in batches of at most NRS_SPP_BATCH_MAX (one launch each) and folded into the running mean, and the last fold is fused with the display
        step (tonemap: `background`, `exposure`, `tonemap_curve`; sRGB output unless `linear`).  Returns a host array [H, W, 4]: float32 for fmt "rgba32f", uint8 for
        "rgba8".  The accumulate buffer stays readable as render_to_cpu_buffer().accumulate_buffer().

        A moving camera: with start_time >= 0 (the reference's own condition, python_api.cu:139) the frame runs from m_smoothed_camera to the (smoothed) camera of
        end_time -- the path's keyframe there, or without keyframes camera_matrix1 (camera_matrix0 when that is None) -- and over a path every sample takes fov, dof and
        focus plane from it at its own time.  Sample i renders between log_space_lerp(start, end, i / spp * shutter_fraction) and (i + 1) / spp * shutter_fraction
        (nrs_motion_views), a view per sample in one launch per batch, and m_smoothed_camera is left at the end camera.

        WHAT camera_matrix1 MEANS with start_time < 0 is decided by `motion_blur`.  False: the still call -- camera_matrix0 / camera_matrix1 go to every sample as they
        are (the two cameras of a rolling shutter) and shutter_fraction is not looked at.  True: camera_matrix1 is the end-of-shutter camera of a frame that starts at
        camera_matrix0, for every shutter_fraction, 1.0 included.  None (the default) is True exactly when shutter_fraction != 1.0: the reference's default shutter
        keeps the call what it was before these arguments existed, bit for bit -- so a full-shutter blur between two cameras has to be asked for with motion_blur=True."""
        spp = int(spp)
        if spp < 1:
            raise ValueError("spp must be at least 1")
        on_path = start_time >= 0.0
        moving = on_path or (float(shutter_fraction) != 1.0 if motion_blur is None else bool(motion_blur))
        buf = self._windowless
        if buf is None or buf.in_resolution() != (int(width), int(height)):
            buf = self._windowless = RenderBuffer(width, height, device=_device(self.ctx))   # m_windowless_render_surface.resize
        buf.set_spp(0)                                                                       # reset_accumulation
        buf.set_color_space(color_space)
        buf.set_tonemap_curve(tonemap_curve)
        if moving:
            start_cam, end_cam, start_time, end_time = self._open_shutter(camera_matrix0, camera_matrix1, on_path, start_time, end_time, fps)
            base = _abi.SampleView()
            base.focal_length[:] = list(focal_length)
            base.dof, base.slice_plane_z = self.dof, self.slice_plane_z + self.scale
        else:
            cam1 = camera_matrix0 if camera_matrix1 is None else camera_matrix1
        done, out = 0, None
        while done < spp:
            k = min(spp - done, _abi.SPP_BATCH_MAX)
            if moving:   # a view per sample
                views = self.motion_views(start_cam, end_cam, shutter_fraction, k, done, spp, (width, height), start_time, end_time, base)
                p = self.make_params(buf, focal_length, views[0].camera_matrix0, views[0].camera_matrix1, rolling_shutter, screen_center, apply_operators and self.enable_edits)
                frames, depths, steps = buf.spp_slabs(k)
                self.render_spp_with_views(network, p, views, frames, depths, steps, None, stream)
            else:
                frames = self.render_nerf_spp(network, buf, k, focal_length, camera_matrix0, cam1, rolling_shutter, screen_center, apply_operators, stream)[0]
            if done + k < spp:
                buf.accumulate_spp(self.ctx, frames, stream, color_space)
            else:
                out = buf.accumulate_spp_tonemap(self.ctx, frames, exposure, background, 0 if linear else 1, fmt, stream)
            done += k
        if moving:
            self._close_shutter(end_cam, on_path, spp, start_time, end_time, shutter_fraction)
        if stream is not None:
            (stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(int(stream))).synchronize()
        return out.cpu().numpy()

    def _open_shutter(self, camera_matrix0, camera_matrix1, on_path, start_time, end_time, fps):
        """The cameras a moving frame of render_to_cpu starts and ends on, with m_camera / m_smoothed_camera moved as the reference moves them -> (start camera,
        end camera, start_time, end_time)"""
        cam0 = [float(v) for v in np.asarray(camera_matrix0, np.float32).reshape(-1)]
        if on_path:                                                    # python_api.cu:133-146
            if end_time < 0.0:
                end_time = start_time
            start_cam = list(self.m_smoothed_camera) if self.m_smoothed_camera is not None else cam0
            if self.m_smoothed_camera is None:
                self.m_smoothed_camera = list(start_cam)
            if not self.camera_path:   # set_camera_from_time leaves m_camera alone without keyframes: the caller's camera is the current one
                self.m_camera = cam0 if camera_matrix1 is None else [float(v) for v in np.asarray(camera_matrix1, np.float32).reshape(-1)]
            self.set_camera_from_time(end_time)
            self.apply_camera_smoothing(1000.0 / fps)
            end_cam = list(self.m_smoothed_camera)
        else:
            start_cam = cam0
            end_cam = cam0 if camera_matrix1 is None else [float(v) for v in np.asarray(camera_matrix1, np.float32).reshape(-1)]
            self.m_camera = list(end_cam)
            start_time = -1.0
        return start_cam, end_cam, start_time, end_time

    def _close_shutter(self, end_cam, on_path, spp, start_time, end_time, shutter_fraction):
        """What a moving frame of render_to_cpu leaves behind on the testbed"""
        if on_path:   # the loop's last set_camera_from_time: the testbed is left on the last sample's keyframe
            a0 = np.float32(spp - 1) / np.float32(spp) * np.float32(shutter_fraction)
            a1 = (np.float32(spp - 1) + np.float32(1.0)) / np.float32(spp) * np.float32(shutter_fraction)
            self.set_camera_from_time(float(np.float32(start_time) + (np.float32(end_time) - np.float32(start_time)) * (a0 + a1) / np.float32(2.0)))
        self.m_smoothed_camera = list(end_cam)                         # python_api.cu:167-168

    def evaluate(self, network, dataset, spp=8, color_space=0, background=(0.0, 0.0, 0.0, 1.0), min_transmittance=1e-4, apply_operators=False, stream=None):
        """The test loop of scripts/run.py --test_transforms (:215-302) over every image of a runtime.Dataset, all of it on the device: the accumulation of a
        RenderBuffer of the dataset's resolution is reset, `spp` samples are rendered in batches of at most NRS_SPP_BATCH_MAX with that image's camera record --
        xform_start as both camera matrices (run.py renders a still camera: set_nerf_camera_matrix), focal_length, principal_point as the screen centre, the record's
        lens distortion, snap_to_pixel_centers on, rendering_min_transmittance = min_transmittance (run.py: 1e-4) -- and folded in the Linear colour space, and
        dataset.image_metrics reads the accumulate buffer where it lies.  No tonemap pass runs: with run.py's black background, exposure 0 and the Identity curve the
        tonemap leaves rgb as it is, and the metrics read rgb alone.  color_space is the colour space of the TRAINING (NRS_COLOR_SRGB: the reference image is blended
        over `background` in sRGB space first), not of the fold.  After the last view ONE synchronisation and one copy of n x 32 bytes.  Returns (summary, records):
        metrics.metrics_summary's dict and a numpy record array (fields of nrs_image_metrics_result), one record per image.  The testbed's own snap_to_pixel_centers,
        rendering_min_transmittance and render_distortion are restored on exit, also on an exception."""
        from . import metrics
        if dataset.ctx is not self.ctx:
            raise NrsError("Testbed.evaluate: the dataset belongs to another context")
        spp, n = int(spp), dataset.n_images
        if spp < 1:
            raise ValueError("spp must be at least 1")
        cameras = [dataset.get_camera(i) for i in range(n)]
        if any(c is None for c in cameras):
            raise NrsError("Testbed.evaluate: a camera has never been set (Dataset.set_camera)")
        dev = _device(self.ctx)
        buf = self._evaluate_surface
        if buf is None or buf.in_resolution() != (dataset.width, dataset.height):
            buf = self._evaluate_surface = RenderBuffer(dataset.width, dataset.height, device=dev)
        s = torch.cuda.current_stream(dev) if stream is None else (stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(int(stream)))
        saved = (self.snap_to_pixel_centers, self.rendering_min_transmittance, self.render_distortion)
        try:
            self.snap_to_pixel_centers, self.rendering_min_transmittance = True, float(min_transmittance)
            with torch.cuda.stream(s):   # (the slabs are cleared by torch: on the stream the launches go to)
                records = torch.empty((n, metrics.RECORD_BYTES), dtype=torch.uint8, device=dev)
                for i, cam in enumerate(cameras):
                    buf.set_spp(0)       # reset_accumulation
                    self.render_distortion = (int(cam.distortion_mode), tuple(cam.distortion_params))
                    matrix = list(cam.xform_start)
                    done = 0
                    while done < spp:
                        k = min(spp - done, _abi.SPP_BATCH_MAX)
                        frames = self.render_nerf_spp(network, buf, k, tuple(cam.focal_length), matrix, matrix, (0.0, 0.0, 0.0, 0.0), tuple(cam.principal_point),
                                                      apply_operators, s)[0]
                        buf.accumulate_spp(self.ctx, frames, s, _abi.COLOR_LINEAR)
                        done += k
                    dataset.image_metrics(i, buf.accumulate_buffer(), color_space, background, out=records[i], stream=s)
                host = torch.empty((n, metrics.RECORD_BYTES), dtype=torch.uint8, pin_memory=True)
                host.copy_(records, non_blocking=True)
            s.synchronize()
        finally:
            self.snap_to_pixel_centers, self.rendering_min_transmittance, self.render_distortion = saved
        recs = metrics.records_from_bytes(host.numpy().copy())
        return metrics.metrics_summary(recs), recs

    def render_to_cpu_buffer(self):
        """The RenderBuffer render_to_cpu renders into (m_windowless_render_surface); None before the first call."""
        return self._windowless

    def get_density_on_grid(self, res3d, aabb_min, aabb_max, mask_with_density_grid=True, stream=None):
        """Testbed::get_density_on_grid(res3d, aabb) (testbed_nerf.cu:4538) -> float32 CUDA tensor [rz, ry, rx]"""
        res, mn, mx = _uint3(res3d), _float3(aabb_min), _float3(aabb_max)
        out = torch.zeros((int(res3d[2]), int(res3d[1]), int(res3d[0])), dtype=torch.float32, device=_device(self.ctx))
        check(self.lib.nrs_density_on_grid(self.nerf_network.h, _stream_handle(stream), C.byref(res), C.byref(mn), C.byref(mx),
                                           1 if mask_with_density_grid else 0, out.data_ptr()))
        return out

    # ---- mesh extraction (Testbed::marching_cubes and its Python callers) ----
    @staticmethod
    def get_marching_cubes_res(res_1d, aabb_min, aabb_max):
        """get_marching_cubes_res(res_1d, aabb) (marching_cubes.cu:48) -> (rx, ry, rz), each a multiple of 16; host-only"""
        out = (C.c_uint32 * 3)()
        check(_abi.load().nrs_marching_cubes_res(int(res_1d), C.byref(_float3(aabb_min)), C.byref(_float3(aabb_max)), C.byref(out)))
        return tuple(out)

    def _mesh_aabb(self, aabb):
        if aabb is None or len(aabb) == 0:   # aabb.is_empty(): the render box (python_api.cu:106-108)
            return self.render_aabb
        return aabb

    def marching_cubes(self, res3d, aabb=None, thresh=_abi.MESH_THRESH_DEFAULT, mask_with_density_grid=True, stream=None):
        """Testbed::marching_cubes(res3d, aabb, thresh) (testbed_nerf.cu:4614): the mesh stays on the testbed (self.mesh, m_mesh); returns the number of triangles."""
        if np.isscalar(res3d):
            res3d = (res3d,) * 3
        mn, mx = self._mesh_aabb(aabb)
        h = C.c_void_p()
        check(self.lib.nrs_mesh_extract(self.nerf_network.h, _stream_handle(stream), C.byref(_uint3(res3d)), C.byref(_float3(mn)),
                                        C.byref(_float3(mx)), float(thresh), 1 if mask_with_density_grid else 0, 1 if self.linear_colors else 0, C.byref(h)))
        if self.mesh is not None:
            self.mesh.close()
        self.mesh = Mesh(self.lib, h)
        return self.mesh.n_tris

    def compute_marching_cubes_mesh(self, res3d=128, aabb=None, thresh=_abi.MESH_THRESH_DEFAULT):
        """Testbed::compute_marching_cubes_mesh (python_api.cu:105-127) -> {"V", "N", "C": float32 [n_verts_padded, 3], "F": int32 [n_tris, 3]}; N normalised on the host"""
        self.marching_cubes(res3d, aabb, thresh)
        V, N, Cc, _, F = self.mesh.download()
        with np.errstate(invalid="ignore", divide="ignore"):
            sq = (N * N).sum(axis=1, dtype=np.float32)
            N = np.where(sq[:, None] > 0, N / np.sqrt(sq, dtype=np.float32)[:, None], N).astype(np.float32)   # Eigen's normalize(): a zero vector stays
        return {"V": V, "N": N, "C": Cc, "F": F.view(np.int32)}

    def compute_and_save_marching_cubes_mesh(self, filename, res3d=128, aabb=None, thresh=_abi.MESH_THRESH_DEFAULT, unwrap_it=False, dataset_offset=(0.0, 0.0, 0.0)):
        """Testbed::compute_and_save_marching_cubes_mesh (testbed.cu:337-343): positions go out as (v - dataset offset) / dataset scale; .ply is a PLY, anything else an OBJ"""
        if unwrap_it:
            raise NrsError("compute_and_save_marching_cubes_mesh: unwrap_it (the UV unwrap and its texture) is not built")
        self.marching_cubes(res3d, aabb, thresh)
        self.mesh.save(filename, self.dataset_scale, dataset_offset)

    def growing_selection(self, max_cascade=0):
        """A GrowingSelection over the model's density grid (m_density_grid copied to the host, as reset_growing does); max_cascade: m_max_cascade"""
        return GrowingSelection(self.ctx, self.nerf_network.get_density_grid(), max_cascade)

    def project_selection_pixels(self, params, pixels_xy, transmittance_threshold=0.1, automatic_max_level=True, growing_level=0, stream=None):
        """GrowingSelection::project_selection_pixels (growing_selection.cu:1832): scribbled pixels -> surface points and the
        occupancy cells they fall into.  Returns (positions [n, 3], cells [n], found [n]) per pixel plus the de-duplicated
        (cells, positions, growing_level) the region growing starts from."""
        px = torch.as_tensor(np.ascontiguousarray(pixels_xy, np.int32).reshape(-1, 2), device=_device(self.ctx))
        n = px.shape[0]
        pos = torch.zeros((n, 3), dtype=torch.float32, device=px.device)
        cells = torch.zeros((n,), dtype=torch.int32, device=px.device)
        found = torch.zeros((n,), dtype=torch.uint8, device=px.device)
        check(self.lib.nrs_project_selection_pixels(self.nerf_network.h, _stream_handle(stream), C.byref(params), px.data_ptr(), n,
                                                    float(transmittance_threshold), pos.data_ptr(), cells.data_ptr(), found.data_ptr()))
        if stream is not None:
            stream.synchronize()
        else:
            torch.cuda.synchronize()
        h_pos, h_cells, h_found = pos.cpu().numpy(), cells.cpu().numpy().view(np.uint32), found.cpu().numpy()
        level = C.c_uint32(int(growing_level))
        out_cells, out_pos, n_out = np.zeros(n, np.uint32), np.zeros((n, 3), np.float32), C.c_uint32()
        check(self.lib.nrs_selection_cells(h_pos.ctypes.data, h_cells.ctypes.data, h_found.ctypes.data, n, 1 if automatic_max_level else 0,
                                           C.byref(level), out_cells.ctypes.data, out_pos.ctypes.data, C.byref(n_out)))
        return (h_pos, h_cells, h_found), (out_cells[: n_out.value], out_pos[: n_out.value], level.value)

    def compute_poisson_boundary(self, vertices, is_inside, jitter, sh_sampling_width=10, hemisphere_width=10):
        """GrowingSelection::compute_poisson_boundary (growing_selection.cu:2220): per cage vertex the density and the SH9 fit of
        the colours around it.  jitter: [n_verts * w * w, 2] in [0, 1] (the reference's std::rand() draws).  -> (density [n], sh [n, 27])"""
        v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
        jt = np.ascontiguousarray(jitter, np.float32)
        n = v.shape[0]
        if jt.size != n * sh_sampling_width * sh_sampling_width * 2:
            raise NrsError("compute_poisson_boundary: jitter must hold two draws per sample")
        density, sh = np.zeros(n, np.float32), np.zeros((n, 27), np.float32)
        check(self.lib.nrs_poisson_boundary(self.nerf_network.h, v.ctypes.data, n, int(sh_sampling_width), int(hemisphere_width), jt.ctypes.data,
                                            1 if is_inside else 0, density.ctypes.data, sh.ctypes.data))
        return density, sh

    def get_rgba_on_grid(self, res3d, ray_dir, stream=None):
        """Testbed::get_rgba_on_grid(res3d, ray_dir) (testbed_nerf.cu:4588) over m_render_aabb -> float32 CUDA tensor [rz, ry, rx, 4]"""
        res, mn, mx, rd = _uint3(res3d), _float3(self.render_aabb[0]), _float3(self.render_aabb[1]), _float3(ray_dir)
        out = torch.zeros((int(res3d[2]), int(res3d[1]), int(res3d[0]), 4), dtype=torch.float32, device=_device(self.ctx))
        check(self.lib.nrs_rgba_on_grid(self.nerf_network.h, _stream_handle(stream), C.byref(res), C.byref(mn), C.byref(mx), C.byref(rd), out.data_ptr()))
        return out

    def new_grid_update(self, max_cascade=0, seed=1337, decay=0.95):
        """The Testbed members update_density_grid_nerf_operator reads: m_rng = default_rng_t{m_seed} (testbed.cu:2220),
        density_grid_ema_step = 0, density_grid_decay = 0.95 (testbed.h:604), sized as update_density_grid_nerf_render does."""
        u = _abi.GridUpdate()
        u.n_uniform_samples = _abi.GRID_VOLUME * (max_cascade + 1)
        u.n_nonuniform_samples = 0
        u.reset_grid = 0
        u.max_cascade = max_cascade
        u.decay = decay
        u.ema_step = 0
        u.rng_state, u.rng_inc = rng_seed(seed)
        return u

    def update_density_grid_nerf_operator(self, update, stream=None, apply_operators=True):
        """Testbed::update_density_grid_nerf_operator (testbed_nerf.cu:3533): one refresh of the occupancy in deformed space."""
        ops = self.edit_operators if (apply_operators and self.enable_edits) else []
        self.nerf_network.update_density_grid(update, ops, stream)

    def update_density_grid_nerf_render(self, n_iterations, reset_grid, update, stream=None):
        """Testbed::update_density_grid_nerf_render (testbed_nerf.cu:3514)."""
        for i in range(n_iterations):
            update.reset_grid = 1 if (reset_grid and i == 0) else 0
            self.update_density_grid_nerf_operator(update, stream)
        update.reset_grid = 0

    def trace_samples(self, p, pixel_idx, max_samples, stream=None):
        """Test hook: (t, dt) stream per listed pixel -> (t [n, max], dt [n, max], count [n]) as CUDA tensors."""
        _require_cuda(pixel_idx, torch.int32, "pixel_idx")
        n = pixel_idx.numel()
        dev = pixel_idx.device
        t = torch.zeros((n, max_samples), dtype=torch.float32, device=dev)
        dt = torch.zeros((n, max_samples), dtype=torch.float32, device=dev)
        cnt = torch.zeros(n, dtype=torch.int32, device=dev)
        check(self.lib.nrs_trace_samples(self.nerf_network.h, C.byref(p), _stream_handle(stream), n, pixel_idx.data_ptr(), max_samples,
                                         t.data_ptr(), dt.data_ptr(), cnt.data_ptr()))
        return t, dt, cnt
