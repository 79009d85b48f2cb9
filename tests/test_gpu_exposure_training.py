"""Trainer(..., exposure=...) on an MI355X: tests/test_gpu_envmap_training.py's rig -- 16 x 12 images, 256 rays, max_samples 2^14, four opaque images.

What "bit for bit" is asserted on.  The exposure's path has no float atomic and the loss of a step is computed before that step's backward pass, so the loss,
dL/doutput and all of the exposure's state are functions of their inputs.  The network's backward pass sums parameter gradients with float atomics, so two identical
steps need not leave the same last bit in every network weight (tests/test_gpu_envmap_training.py's docstring).  Therefore: at the default learning rate ONE step
with cam_update_every = 1 -- the update falls inside it, the exposures move -- is compared in every bit (loss, dL/doutput, exposure state); and 17 steps with the
default cadence, so that the update of the 16th falls inside, are compared in every bit at network learning rate 0, the network's weights included.  The exposure's
learning rate is the network's, so in that run the update changes the moments, the step count and the cells, and the values by the renormalisation alone: the
exposures there are set to non-zero values beforehand, so that every target is scaled."""
import math

import numpy as np
import pytest
import torch

import envmap_ref
import exposure_ref as ref

from training_rig import N_IMAGES, N_RAYS, after_step, bits, by_hand, exposure_state, make_dataset, make_rig, make_trainer, new_exposure, step_rays

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def rig(built):
    return make_rig()


def test_step_is_the_calls_made_by_hand(rig):
    from nerfshop_amd import _abi
    ds = rig[2]
    start = np.random.default_rng(2).uniform(-1.0, 1.0, (N_IMAGES, 3)).astype(f32)
    # the default learning rate, an update on every step: one step, the exposures move
    a, b = (make_trainer(rig, exposure=new_exposure(rig, start), cam_update_every=1) for _ in range(2))
    rays, jitter, target, background, pixels = step_rays(ds, a, want_pixels=True)
    loss_a = a.step(rays, target, jitter=jitter, background=background, pixels=pixels)
    loss_b, dl_b = by_hand(b, [0], rays, target, jitter, background, pixels)
    torch.cuda.synchronize()
    assert math.isfinite(float(loss_a)) and float(loss_a) > 0 and bits(loss_a) == bits(loss_b)
    assert bits(a._bufs.dl) == bits(dl_b), "dL/doutput: what the backward pass is given"
    assert exposure_state(a) == exposure_state(b)
    values = a.exposures()
    assert a.exposure.step_count() == 1 and (values != start).all() and not a.exposure.get(_abi.EXPOSURE_CELLS).any(), "the exposures moved, the cells are clear"
    assert np.abs(values.astype(np.float64).sum(axis=0)).max() <= N_IMAGES * np.spacing(f32(np.abs(values).max())), "zero mean"
    # network learning rate 0, the default cadence: 17 steps, everything in every bit
    a, b = (make_trainer(rig, learning_rate=0.0, exposure=new_exposure(rig, start)) for _ in range(2))
    hand = [0]
    for k in range(17):
        rays, jitter, target, background, pixels = step_rays(ds, a, want_pixels=True)
        loss_a = a.step(rays, target, jitter=jitter, background=background, pixels=pixels)
        loss_b, dl_b = by_hand(b, hand, rays, target, jitter, background, pixels)
        after_step((a, b))
        torch.cuda.synchronize()
        assert bits(loss_a) == bits(loss_b) and bits(a._bufs.dl) == bits(dl_b), k
        assert exposure_state(a) == exposure_state(b), k
        assert a.exposure.step_count() == (1 if k >= 15 else 0), "the update falls on the 16th step"
        assert bool(a.exposure.get(_abi.EXPOSURE_CELLS).any()) == (k != 15), "the cells fill between updates and are clear behind one"
    assert a.exposure.get(_abi.EXPOSURE_M).any() and a.exposure.get(_abi.EXPOSURE_V).any(), "the update ran: the moments moved"
    for which in (_abi.OPT_MASTER, _abi.OPT_PARAMS_FP16):
        assert a.optimizer.get_state(which).tobytes() == b.optimizer.get_state(which).tobytes()


def test_without_an_exposure_nothing_changes(rig):
    """Trainer(exposure=None) computes what a Trainer built without the argument computes: the losses of four dataset steps bit for bit at network learning rate 0,
    and the network's parameters behind them."""
    from nerfshop_amd import _abi
    ds = rig[2]
    plain, none = make_trainer(rig, learning_rate=0.0), make_trainer(rig, learning_rate=0.0, exposure=None, exposure_l2_reg=0.0, cam_update_every=16)
    for k in range(4):
        la, lb = plain.step_dataset(ds, N_RAYS), none.step_dataset(ds, N_RAYS)
        torch.cuda.synchronize()
        assert math.isfinite(float(la)) and float(la) > 0 and bits(la) == bits(lb), k
        assert bits(plain._bufs.dl) == bits(none._bufs.dl)
    assert none.exposure is None and none.exposures() is None and none._bufs.target is None and none._bufs.scale is None and none._bufs.aux is None
    for which in (_abi.OPT_MASTER, _abi.OPT_PARAMS_FP16):
        assert plain.optimizer.get_state(which).tobytes() == none.optimizer.get_state(which).tobytes()


def test_the_update(rig, monkeypatch):
    """Two opaque images of bytes 240 and 20, no random background, a mid-grey background, linear colours.  The exposures stay exactly zero for the steps 0..15 and
    change at the 16th.  A fresh network's colour lies between the two images' (a logistic of small numbers over grey), and 16 steps do not carry it past either, so
    dL/dC is negative on the bright image and positive on the dark one: the bright image's exposure gradient -dL/dC * scale * ln2 is positive, the dark one's
    negative.  That is checked first, with the twin on the device's own records of every step (taken where Trainer hands them to Exposure.accumulate): the twin's
    cells are the device's bit for bit before the 16th step, and the signs of the 16 steps' sum are those.  Then the first update: the bright image's exposures
    negative, the dark one's positive, bit-equal to the host twin of the step on those cells, and their sum zero within one float32 step."""
    from nerfshop_amd import _abi, runtime
    from nerfshop_amd.torch_module import LOSS_SCALE
    ds = make_dataset(rig[0], [(240, 240, 240), (20, 20, 20)])
    lp = _abi.RayLossParams(loss_scale=LOSS_SCALE, background=(0.5, 0.5, 0.5), train_in_linear_colors=1)
    t = make_trainer(rig, exposure=True, loss_params=lp)
    records = []
    inner = runtime.Exposure.accumulate

    def recording(self, params, ray_counter, ray_indices, numsteps_out, aux, scale, xy_pdf=None, n_rays=None, stream=None):
        records.append([x.clone() for x in (ray_counter, ray_indices, numsteps_out, aux, scale)] + [xy_pdf, n_rays, float(params.loss_scale), params.train_in_linear_colors])
        return inner(self, params, ray_counter, ray_indices, numsteps_out, aux, scale, xy_pdf=xy_pdf, n_rays=n_rays, stream=stream)
    monkeypatch.setattr(runtime.Exposure, "accumulate", recording)
    assert t.exposure is True
    for k in range(15):
        loss = t.step_dataset(ds, N_RAYS, random_bg=False)
        assert isinstance(t.exposure, runtime.Exposure), "exposure=True becomes a handle on the first dataset step"
        assert not t.exposures().any() and t.exposure.step_count() == 0, f"step {k}: the exposures stay exactly zero"
    assert math.isfinite(float(loss)) and t.exposure.n_images == 2 and t.exposure.params.steps_between_updates == 16
    device_cells = [int(c) for c in t.exposure.get(_abi.EXPOSURE_CELLS).reshape(-1)]
    lr = t.current_learning_rate()
    t.step_dataset(ds, N_RAYS, random_bg=False)
    values = t.exposures()
    assert len(records) == 16 and t.exposure.step_count() == 1 and not t.exposure.get(_abi.EXPOSURE_CELLS).any()
    # the twin on the device's records
    cells = None
    for k, (counter, idx, numsteps_out, aux, scale, xy_pdf, n_rays, loss_scale, lin) in enumerate(records):
        assert xy_pdf is None and n_rays == N_RAYS and lin == 1
        cells = ref.accumulate_cells(N_RAYS, 2, int(counter.cpu()[0]), idx.cpu().numpy(), numsteps_out.cpu().numpy(), envmap_ref.split_aux(aux.cpu().numpy()),
                                     scale.cpu().numpy(), None, loss_scale, True, cells=cells)
        if k == 14:
            assert cells == device_cells, "before the 16th step the device's cells are the twin's"
    print("accumulated exposure gradient (bright | dark):", envmap_ref.cells_to_gradient(cells))
    assert all(c > 0 for c in cells[:3]) and all(c < 0 for c in cells[3:]), "the bright image's gradient is positive, the dark one's negative"
    z = np.zeros((2, 3), f32)
    host = runtime.exposure_step_host(np.asarray(cells, np.int64).reshape(2, 3), z, z, z, 0, LOSS_SCALE, lr)
    assert values.tobytes() == host[1].tobytes(), "the update is the host twin's on those cells"
    print("exposures after the first update (bright | dark):", values.reshape(-1))
    assert (values[0] < 0).all() and (values[1] > 0).all()
    assert (np.abs(values[0].astype(np.float64) + values[1].astype(np.float64)) <= np.spacing(np.abs(values).max(axis=0))).all(), "they sum to zero within one float32 step"


def test_refusals(rig):
    from nerfshop_amd import trainer as tr
    from nerfshop_amd._abi import NrsError
    ds = rig[2]
    t = make_trainer(rig, exposure=new_exposure(rig))
    rays, jitter, target, background, pixels = step_rays(ds, t, want_pixels=True)
    with pytest.raises(NrsError, match="pixels"):
        t.step(rays, target, jitter=jitter, background=background)
    t = make_trainer(rig, exposure=True)
    with pytest.raises(NrsError, match="pixel's density alone"):
        t.step_dataset(ds, N_RAYS, error_map=tr.ErrorMapSchedule(sample_images=True, sample_pixels=True))
    with pytest.raises(NrsError, match="step_dataset"):
        t.step(rays, target, jitter=jitter, background=background, pixels=pixels)
    with pytest.raises(NrsError, match="number of images"):
        make_trainer(rig, exposure=new_exposure(rig, n_images=3)).step_dataset(ds, N_RAYS)
    with pytest.raises(NrsError, match="exposure must be"):
        make_trainer(rig, exposure=(4, 3))
    # the combinations that are served: pixel sampling alone hands the pdf over, image sampling alone does not
    for kw in (dict(sample_pixels=True), dict(sample_images=True), dict()):
        t = make_trainer(rig, exposure=True)
        em = tr.ErrorMapSchedule(steps_between=2, **kw)
        losses = [float(t.step_dataset(ds, N_RAYS, error_map=em)) for _ in range(4)]
        assert all(math.isfinite(x) and x > 0 for x in losses) and em.builds >= 1 and np.isfinite(t.exposures()).all()
