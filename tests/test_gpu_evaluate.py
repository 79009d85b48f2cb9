"""Testbed.evaluate and Trainer.evaluate on an MI355X: run.py's test loop on the device, against tests/metrics_ref.py applied to what render_to_cpu returns for the
same cameras and to the dataset's own stored images.

The test set: 3 views of 24 x 16 of the `scene` fixture, each rendered by render_to_cpu at 8 spp over a black background, quantised to 8-bit sRGB, fed to a
runtime.Dataset as uint8, with cameras in TrainingCamera form.  evaluate's records are held to the restatement with the bars of tests/test_metrics_host.py.  Every
PSNR is at least 50 dB: the 8-bit quantisation alone gives 58.9 dB (a uniform error of half a level: 20 log10(255 sqrt(12))) and fp16 storage moves an sRGB value by
at most 2e-4, so a lower figure means the camera mapping is wrong.  Repeated with a view whose principal point is not the image's centre.

Trainer.evaluate after 4 fit steps: finite numbers; ema=True renders other parameters than ema=False; and training state is untouched.  The backward pass sums
parameter gradients with float atomics, so two fits do not agree bit for bit at the default learning rate, with or without an evaluation between them
(tests/test_gpu_error_map.py, test_fit_observes_and_does_not_steer).  "The next step's loss is the loss without the evaluation, bit for bit" is therefore asserted in the
two ways that are functions of their inputs: every array of the optimiser, the fp16 parameters, the density grid, the generator and the counters are the same bytes
after the evaluation as before it (the next step's loss is computed from exactly these, in a forward pass without atomics); and at learning rate 0, where fit is a
function of its inputs, the fifth step's loss with an evaluation after the fourth equals the fifth step's loss without, in every bit."""
import math

import numpy as np
import pytest

import metrics_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, H, SPP = 24, 16, 8
BLACK = (0.0, 0.0, 0.0, 1.0)
f32 = np.float32


def make_test_set(rig, views):
    """views: (azimuth, principal point) -> (dataset, [render_to_cpu(linear=True) of each view])"""
    from nerfshop_amd import _abi, runtime, synth
    tb = rig.testbed
    rig.use_edit(False)
    focal = 0.5 * W / math.tan(0.5 * synth.CAMERA_ANGLE_X)
    ds = runtime.Dataset(rig.ctx, len(views), W, H)
    linear = []
    saved = tb.rendering_min_transmittance
    tb.rendering_min_transmittance = 1e-4   # what evaluate renders with
    try:
        for k, (azimuth, pp) in enumerate(views):
            camera = rig.scene.camera(azimuth)
            srgb8 = tb.render_to_cpu(rig.net, W, H, SPP, False, (focal, focal), camera, screen_center=pp, background=BLACK, fmt="rgba8", apply_operators=False)
            assert srgb8.dtype == np.uint8 and (srgb8[..., 3] == 255).all() and srgb8[..., :3].max() > 64, "the view shows the scene, composited on black"
            ds.set_image(k, srgb8)
            cam = _abi.TrainingCamera()
            cam.xform_start[:] = cam.xform_end[:] = camera.tolist()
            cam.focal_length[:], cam.principal_point[:] = (focal, focal), pp
            ds.set_camera(k, cam)
            linear.append(tb.render_to_cpu(rig.net, W, H, SPP, True, (focal, focal), camera, screen_center=pp, background=BLACK, apply_operators=False))
    finally:
        tb.rendering_min_transmittance = saved
    return ds, linear


@pytest.mark.parametrize("views", [[(20.0, (0.5, 0.5)), (140.0, (0.5, 0.5)), (260.0, (0.5, 0.5))], [(20.0, (0.5, 0.5)), (140.0, (0.41, 0.57)), (260.0, (0.5, 0.5))]],
                         ids=["centred", "principal_point"])
def test_evaluate_against_render_to_cpu(rig, views):
    import torch
    from nerfshop_amd import runtime
    from nerfshop_amd._abi import NrsError
    tb = rig.testbed
    ds, linear = make_test_set(rig, views)
    before = (tb.snap_to_pixel_centers, tb.rendering_min_transmittance, tb.render_distortion)
    tb.snap_to_pixel_centers = False   # evaluate snaps, and puts this back
    try:
        summary, records = tb.evaluate(rig.net, ds, spp=SPP)
        assert (tb.snap_to_pixel_centers, tb.rendering_min_transmittance, tb.render_distortion) == (False,) + before[1:], "the testbed's own settings are restored"
        with pytest.raises(NrsError):
            tb.evaluate(rig.net, ds, spp=SPP, color_space=0, background=(0.0, float("nan"), 0.0, 1.0))
        assert (tb.snap_to_pixel_centers, tb.rendering_min_transmittance, tb.render_distortion) == (False,) + before[1:], "also on an exception"
    finally:
        tb.snap_to_pixel_centers = before[0]
    assert len(records) == 3 and summary["n_views"] == 3
    for k in range(3):
        want = ref.metrics(linear[k], ds.get_image(k).astype(f32), ref.COLOR_LINEAR, BLACK)
        d_ssim = abs(float(records["ssim"][k]) - float(want["ssim"]))
        d_mse = abs(float(records["mse"][k]) - float(want["mse"])) / float(want["mse"])
        print(f"view {k}: psnr {float(records['psnr'][k]):.3f} dB (restatement {float(want['psnr']):.3f}), ssim {float(records['ssim'][k]):.6f}, |d ssim| {d_ssim:.2e}, mse rel {d_mse:.2e}")
        assert int(records["n_pixels"][k]) == W * H
        assert d_ssim <= ref.SSIM_BAR and d_mse <= ref.MSE_BAR
        assert float(records["psnr"][k]) >= 50.0, "the camera record maps to another view than the one the image shows"
    want = ref.summary(records["mse"], records["ssim"], records["psnr"])
    assert all(abs(summary[k] - want[k]) <= 1e-12 * abs(want[k]) for k in ("psnr_mean", "psnr_min", "psnr_max", "ssim_mean", "psnr_avgmse"))
    # a dataset of another context is refused before anything is rendered
    other = runtime.Context(0)
    ds_other = runtime.Dataset(other, 1, W, H)
    with pytest.raises(NrsError, match="another context"):
        tb.evaluate(rig.net, ds_other)
    ds_other.close()
    torch.cuda.synchronize()
    ds.close()


def training_state(trainer):
    from nerfshop_amd import _abi
    opt = trainer.optimizer
    u = trainer._grid_update
    arrays = [opt.get_state(w).tobytes() for w in (_abi.OPT_MASTER, _abi.OPT_M, _abi.OPT_V, _abi.OPT_STEPS, _abi.OPT_EMA, _abi.OPT_PARAMS_FP16)]
    arrays += [trainer.network.get_density_grid().tobytes(), trainer.network.get_density_bitfield().tobytes(), trainer.grad.cpu().numpy().tobytes()]
    return arrays, (opt.step_count(), trainer.training_step, trainer.n_rays_total, int(u.rng_state), int(u.rng_inc), int(u.ema_step), trainer._grid_step)


def test_trainer_evaluate_leaves_training_alone(rig):
    import torch
    from nerfshop_amd import _abi, synth
    from nerfshop_amd.trainer import Trainer
    ds, _ = make_test_set(rig, [(20.0, (0.5, 0.5)), (140.0, (0.5, 0.5)), (260.0, (0.5, 0.5))])
    desc14 = synth.model_desc(log2_hashmap_size=14)
    grid = synth.density_grid(1)

    def trainer_after_4(learning_rate):
        t = Trainer(rig.ctx, desc14, seed=11, density_grid=grid, max_samples=1 << 17, learning_rate=learning_rate)
        t.fit(ds, 4, n_rays=1024)
        torch.cuda.synchronize()
        return t

    t = trainer_after_4(_abi.BASE_LEARNING_RATE)
    state = training_state(t)
    summary, records = t.evaluate(ds, spp=2)
    summary_ema, records_ema = t.evaluate(ds, ema=True, spp=2)
    assert training_state(t) == state, "an evaluation changed the training state"
    for s in (summary, summary_ema):
        assert all(math.isfinite(v) for v in s.values()) and s["n_views"] == 3 and 0.0 < s["psnr_mean"] < 60.0
    assert records.tobytes() != records_ema.tobytes(), "the EMA parameters render the picture of the live ones"
    print(f"after 4 steps: live {summary['psnr_mean']:.3f} dB / ssim {summary['ssim_mean']:.4f}, EMA {summary_ema['psnr_mean']:.3f} dB / ssim {summary_ema['ssim_mean']:.4f}")
    loss5 = t.fit(ds, 1, n_rays=1024)[0]
    assert math.isfinite(float(loss5)) and t.training_step == 5

    plain, observed = trainer_after_4(0.0), trainer_after_4(0.0)
    observed.evaluate(ds, spp=2)
    observed.evaluate(ds, ema=True, spp=2)
    a, b = plain.fit(ds, 1, n_rays=1024)[0], observed.fit(ds, 1, n_rays=1024)[0]
    torch.cuda.synchronize()
    assert math.isfinite(float(a)) and float(a) > 0 and torch.equal(a.reshape(1).view(torch.int32), b.reshape(1).view(torch.int32)), (float(a), float(b))
    ds.close()
