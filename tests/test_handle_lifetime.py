"""Handle lifetime of every harness class that owns an ABI object: close() frees it and leaves `h` falsy, a second close() and the destructor are no-ops.

Only closed objects are closed again here; nothing is used after close() and no child outlives its context."""
import numpy as np
import pytest


def close_twice(obj):
    assert obj.h
    obj.close()
    assert not obj.h
    obj.close()
    assert not obj.h
    del obj


@pytest.fixture(scope="module")
def ctx(built):
    import torch
    from nerfshop_amd import runtime
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    c = runtime.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
def test_context(built):
    from nerfshop_amd import runtime
    close_twice(runtime.Context(0))


@pytest.mark.gpu
def test_network(ctx):
    from nerfshop_amd import runtime, synth
    close_twice(runtime.NerfNetwork(ctx, synth.model_desc(1), cell_cache_bytes=0))


@pytest.mark.gpu
def test_unbound_optimizer(ctx):
    from nerfshop_amd import runtime
    close_twice(runtime.Optimizer(ctx, n_params=8, n_matrix=2))


@pytest.mark.gpu
def test_dataset(ctx):
    from nerfshop_amd import runtime
    close_twice(runtime.Dataset(ctx, 1, 8, 8))


@pytest.mark.gpu
def test_cage_deformation(ctx):
    from nerfshop_amd import runtime, synth
    close_twice(runtime.CageDeformation(ctx, synth.model_desc(1), synth.make_cage_edit(lattice_n=4)))


@pytest.mark.gpu
def test_affine_duplication(ctx):
    from nerfshop_amd import runtime, synth
    op = runtime.AffineDuplication(ctx, synth.model_desc(1), synth.make_affine_edit())
    assert callable(op.map_rays) and callable(op.map_positions)
    close_twice(op)


@pytest.mark.gpu
def test_mesh(ctx):
    import torch
    from nerfshop_amd import runtime
    a = np.arange(16, dtype=np.float32) - 7.5
    field = 5.0 - np.sqrt(a[:, None, None] ** 2 + a[None, :, None] ** 2 + a[None, None, :] ** 2)   # a ball of radius 5 cells
    mesh = runtime.mesh_from_density(ctx, torch.as_tensor(field, device="cuda:0"), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 0.0)
    assert mesh.n_tris > 0
    close_twice(mesh)


def test_growing_selection(built):
    from nerfshop_amd import _abi, runtime
    close_twice(runtime.GrowingSelection(None, np.zeros(_abi.GRID_VOLUME * _abi.GRID_CASCADES, np.float32)))
