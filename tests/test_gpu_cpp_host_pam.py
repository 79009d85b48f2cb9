"""render_from_files --pam: the C++ host (nrs_compat.hpp's RenderBuffer::accumulate + tonemap, no Python in its process) writes the 8-bit display image of its frame
as a binary PAM; the bytes equal RenderBuffer.tonemap(fmt="rgba8") of the Python host for the same files and camera.  Without the flag the program runs as before."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "render_from_files")

pytestmark = pytest.mark.gpu


def read_pam(path):
    """-> uint8 [H, W, DEPTH]; the header must be the seven lines of a P7 RGB_ALPHA file"""
    blob = open(path, "rb").read()
    end = blob.index(b"ENDHDR\n") + len(b"ENDHDR\n")
    lines = blob[:end].decode("ascii").splitlines()
    assert lines[0] == "P7" and lines[-1] == "ENDHDR"
    head = dict(line.split(" ", 1) for line in lines[1:-1])
    assert set(head) == {"WIDTH", "HEIGHT", "DEPTH", "MAXVAL", "TUPLTYPE"}
    assert head["DEPTH"] == "4" and head["MAXVAL"] == "255" and head["TUPLTYPE"] == "RGB_ALPHA"
    w, h = int(head["WIDTH"]), int(head["HEIGHT"])
    assert len(blob) - end == w * h * 4
    return np.frombuffer(blob, np.uint8, offset=end).reshape(h, w, 4)


def test_pam_equals_the_python_hosts_rgba8(rig, tmp_path):
    from nerfshop_amd import formats, runtime, synth
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples")])
    scene = rig.scene
    W, H = 131, 73   # odd: a row of the PAM is no multiple of anything
    formats.save_snapshot(tmp_path / "scene.ingp", scene.desc, 1, scene.params, scene.edited_grid, camera=scene.camera(60.0))
    formats.save_edits(tmp_path / "edits.json", [scene.edit])
    tail = [str(tmp_path / "scene.ingp"), str(tmp_path / "edits.json"), str(W), str(H), repr(synth.CAMERA_ANGLE_X)]
    r = subprocess.run([EXE, "--pam", str(tmp_path / "o.pam")] + tail + [str(tmp_path / "o.raw")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout)["n_rays_hit"] > 300
    pam = read_pam(tmp_path / "o.pam")
    assert pam.shape == (H, W, 4)

    # the Python host on the same files (as tests/test_gpu_cpp_host.py sets it up): render, accumulate 1 spp, tonemap to 8 bits with the program's settings
    snap = formats.load_snapshot(tmp_path / "scene.ingp")
    tb = runtime.Testbed(rig.ctx, snap.desc, snap.aabb_scale)
    tb.nerf_network.set_params(snap.params)
    tb.nerf_network.set_density_grid(snap.density_grid)
    tb.add_edit_operator(runtime.CageDeformation(rig.ctx, snap.desc, formats.load_edits(tmp_path / "edits.json")[0], device_authoring=True))
    p = synth.render_params(W, H, snap.camera)
    p.poisson_target = 1
    buf = runtime.RenderBuffer(W, H)
    tb.render_with_params(tb.nerf_network, p, buf.frame_buffer(), buf.depth_buffer(), None, None)
    buf.accumulate(rig.ctx)
    rgba8 = buf.tonemap(rig.ctx, exposure=0.0, background=(0, 0, 0, 0), output_color_space=1, fmt="rgba8")
    rig.torch.cuda.synchronize()
    want = rgba8.cpu().numpy()
    assert want.dtype == np.uint8 and want.shape == (H, W, 4)
    assert np.array_equal(pam, want), f"{int((pam != want).sum())} bytes differ"
    assert pam[..., 3].max() > 200 and pam[..., 3].min() == 0 and len(np.unique(pam[..., :3])) > 50   # a picture, not a constant
    raw_with = np.fromfile(tmp_path / "o.raw", np.float32)
    assert np.array_equal(raw_with[:W * H * 4].reshape(H, W, 4), buf.frame_buffer().cpu().numpy())   # the float frame is written as before, untouched by the display step

    # without the flag: as it runs today, the same out.raw and no PAM
    r = subprocess.run([EXE] + tail + [str(tmp_path / "plain.raw")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.fromfile(tmp_path / "plain.raw", np.float32).view(np.uint32), raw_with.view(np.uint32))
    assert sorted(f.name for f in tmp_path.iterdir() if f.suffix == ".pam") == ["o.pam"]
