"""Host-side mirror of the reference's operator surface for the render path, over the C-ABI of libnrs.so.

Names, argument meaning and error behaviour follow the reference classes so call sites read the same:

    NerfNetwork            <- ngp::NerfNetwork<T> / NerfNetworkFull<T>   include/neural-graphics-primitives/nerf_network.h:86
    CageDeformation        <- ngp::CageDeformation : EditOperator        include/.../editing/edit_operator.h:25, cage_deformation.cu:547
    RenderBuffer           <- ngp::CudaRenderBuffer (frame_buffer / depth_buffer / spp / clear_frame)   render_buffer.h:164
    Testbed.render_nerf    <- Testbed::render_nerf                        src/testbed_nerf.cu:3066

PyTorch is plumbing only: device memory (torch tensors), streams.  All arithmetic happens in the HIP kernels;
there is no CPU path -- a missing library or GPU raises NrsError.

One module per subsystem of the library (the nrs_api_*.cpp it fronts); this file only gathers their names.
"""
from .._abi import NrsError, RenderParams, RenderStats, check
from ._base import _require_cuda, _stream_handle
from .context import Context
from .dataset import Dataset, error_map_cdfs_host, error_map_resolution
from .edits import AffineDuplication, CageDeformation
from .envmap import Envmap
from .exposure import Exposure, exposure_step_host
from .mesh import Mesh, mesh_from_density
from .metrics import image_metrics, image_metrics_host, metrics_summary
from .network import DEFAULT_CELL_CACHE_BYTES, NerfNetwork, rng_advance, rng_seed
from .optimizer import Optimizer, adam_bias_table, exponential_decay_lr
from .render_buffer import RenderBuffer
from .selection import GrowingSelection, bitfield_morph, bitfield_morph_host
from .testbed import Testbed, set_camera_extras
