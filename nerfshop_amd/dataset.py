"""The part of load_nerf (src/nerf_loader.cu:164-640) a `transforms.json` folder needs: cameras and metadata on the host, images decoded with PIL.

    loaded = dataset.load_transforms("data/nerf/fox")             # a folder with a transforms.json, or the file itself
    ds = loaded.to_device(ctx)                                   # runtime.Dataset: images converted on the device, one camera record per image
    trainer.fit(ds, 1000)

Keys read: camera_angle_x / _y, fl_x / _y, cx, cy, w, h, k1 k2 p1 p2, ftheta_p0..p4, rolling_shutter, aabb_scale, scale, offset, white_transparent, black_transparent,
n_frames; per frame file_path and transform_matrix or transform_matrix_start / _end.  Not read: per-frame fovs, sharpness, depth, explicit rays,
envmaps, light directions, `aabb`, `up`, masks and alpha files, EXR.
"""
import json
import math
import os

import numpy as np

from . import _abi, synth
from ._abi import NrsError

NERF_SCALE = 0.33  # nerf_loader.cu:60


class LoadedDataset:
    """What load_transforms returns: cameras (a list of _abi.TrainingCamera), images (a list of [h, w, 4] uint8 sRGB arrays with straight alpha, or None),
    width, height, aabb_scale, scale, offset, white_transparent, black_transparent, paths."""

    def __init__(self):
        self.cameras, self.images, self.paths = [], None, []
        self.width = self.height = 0
        self.aabb_scale, self.scale, self.offset = 1, NERF_SCALE, (0.5, 0.5, 0.5)
        self.white_transparent = self.black_transparent = False

    @property
    def n_images(self):
        return len(self.cameras)

    def to_device(self, ctx, stream=None):
        """A runtime.Dataset holding these images and cameras."""
        from . import runtime
        if self.images is None:
            raise NrsError("LoadedDataset.to_device: loaded without images (load_images=False)")
        ds = runtime.Dataset(ctx, self.n_images, self.width, self.height)
        flags = (_abi.IMAGE_WHITE_TRANSPARENT if self.white_transparent else 0) | (_abi.IMAGE_BLACK_TRANSPARENT if self.black_transparent else 0)
        for i, (img, cam) in enumerate(zip(self.images, self.cameras)):
            ds.set_image(i, img, flags=flags, stream=stream)
            ds.set_camera(i, cam)
        return ds


def _fov_to_focal_length(resolution, degrees):  # common_device.cuh:444, in float32
    f = np.float32
    return f(f(0.5) * f(resolution)) / f(math.tan(f(f(f(0.5) * f(degrees)) * f(3.14159265358979323846)) / f(180)))


def _image_path(base, file_path):
    path = os.path.join(base, file_path)
    if os.path.splitext(path)[1] == "":
        path += ".png"
    return path


def load_transforms(path, load_images=True):
    """Read a transforms.json (or the folder that holds one).  Cameras go through synth.nerf_matrix_to_ngp with the file's scale and offset.  load_images=False returns
    cameras and metadata only (the resolution then comes from the file's w and h)."""
    from PIL import Image
    if os.path.isdir(path):
        path = os.path.join(path, "transforms.json")
    try:
        with open(path) as f:
            js = json.load(f)
    except (OSError, ValueError) as e:
        raise NrsError(f"load_transforms: cannot read {path}: {e}")
    if not isinstance(js.get("frames"), list) or not js["frames"]:
        raise NrsError(f"load_transforms: {path} has no frames")
    base = os.path.dirname(os.path.abspath(path))
    frames = js["frames"]
    if "n_frames" in js:
        frames = frames[:min(len(frames), int(js["n_frames"]))]
    out = LoadedDataset()
    out.white_transparent, out.black_transparent = bool(js.get("white_transparent", False)), bool(js.get("black_transparent", False))
    out.aabb_scale = int(js.get("aabb_scale", 1))
    out.scale = float(js.get("scale", NERF_SCALE))
    if "offset" in js:
        o = js["offset"]
        out.offset = tuple(float(x) for x in o) if isinstance(o, list) else (float(o),) * 3
    out.paths = [_image_path(base, fr["file_path"]) for fr in frames]

    if load_images:
        out.images = []
        for p in out.paths:
            try:
                with Image.open(p) as im:
                    a = np.ascontiguousarray(np.asarray(im.convert("RGBA"), dtype=np.uint8))
            except (OSError, ValueError) as e:
                raise NrsError(f"load_transforms: cannot open image {p}: {e}")
            if out.images and a.shape != out.images[0].shape:
                raise NrsError(f"load_transforms: {p} is {a.shape[1]} x {a.shape[0]}, the images before it are {out.images[0].shape[1]} x {out.images[0].shape[0]}")
            out.images.append(a)
        out.height, out.width = out.images[0].shape[:2]
    else:
        if "w" not in js or "h" not in js:
            raise NrsError(f"load_transforms: {path} names no resolution (w, h) and the images are not loaded")
        out.width, out.height = int(js["w"]), int(js["h"])

    # the camera model, common to every frame (nerf_loader.cu:332-398)
    f32 = np.float32
    mode, params = 0, [0.0] * 7
    for k, name in enumerate(("k1", "k2", "p1", "p2")):
        if name in js:
            params[k] = float(js[name])
            if f32(params[k]) != 0:
                mode = 1
    pp = [0.5, 0.5]
    if "cx" in js:
        pp[0] = f32(js["cx"]) / f32(js["w"])
    if "cy" in js:
        pp[1] = f32(js["cy"]) / f32(js["h"])
    rs = [0.0] * 4
    if "rolling_shutter" in js:
        r = js["rolling_shutter"]
        rs = [float(r[0]), float(r[1]), float(r[2]), float(r[3]) if len(r) >= 4 else 0.0]
    if "ftheta_p0" in js:
        params = [float(js[f"ftheta_p{k}"]) for k in range(5)] + [float(js["w"]), float(js["h"])]
        mode = 2

    def focal(resolution, axis):  # read_focal_length, nerf_loader.cu:579-589 (without the per-frame fovs)
        if f"fl_{axis}" in js:
            return f32(js[f"fl_{axis}"])
        if f"camera_angle_{axis}" in js:
            return _fov_to_focal_length(resolution, f32(f32(f32(js[f"camera_angle_{axis}"]) * f32(180)) / f32(3.14159265358979323846)))
        return f32(0)

    fx, fy = focal(out.width, "x"), focal(out.height, "y")
    if fx != 0:
        fl = (fx, fy if fy != 0 else fx)
    elif fy != 0:
        fl = (fy, fy)
    else:
        raise NrsError(f"load_transforms: {path} names no focal length (fl_x / fl_y / camera_angle_x / camera_angle_y)")

    for fr in frames:
        start = fr["transform_matrix_start"] if "transform_matrix_start" in fr else fr.get("transform_matrix")
        if start is None:
            raise NrsError(f"load_transforms: frame {fr.get('file_path')} has no transform_matrix")
        end = fr.get("transform_matrix_end", start)
        cam = _abi.TrainingCamera()
        cam.xform_start[:] = synth.nerf_matrix_to_ngp(start, out.scale, out.offset).T.reshape(-1).tolist()  # column-major
        cam.xform_end[:] = synth.nerf_matrix_to_ngp(end, out.scale, out.offset).T.reshape(-1).tolist()
        cam.focal_length[:] = [float(fl[0]), float(fl[1])]
        cam.principal_point[:] = [float(pp[0]), float(pp[1])]
        cam.rolling_shutter[:] = rs
        cam.distortion_mode = mode
        cam.distortion_params[:] = params
        out.cameras.append(cam)
    return out
