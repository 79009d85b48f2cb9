"""nrs_ctx (nrs_api.cpp): the device a harness object lives on and the render launch knobs."""
import ctypes as C

from .. import _abi
from .._abi import check
from ._base import Handle


class Context(Handle):
    _destroy = "nrs_ctx_destroy"

    def __init__(self, device=0):
        super().__init__(_abi.load())
        check(self.lib.nrs_ctx_create(int(device), C.byref(self.h)))
        self.device = int(device)
        name = C.create_string_buffer(256)
        ncu, hbm = C.c_int(), C.c_size_t()
        check(self.lib.nrs_ctx_device_info(self.h, name, 256, C.byref(ncu), C.byref(hbm)))
        self.device_name, self.n_cus, self.hbm_bytes = name.value.decode(), ncu.value, hbm.value

    def set_lane_teams(self, lanes_per_ray):
        """0 = automatic (default), 1 / 2 / 4 = lanes of a wavefront per ray in render launches, -1 = hybrid, -2 / -3 / -4 = small-launch schedule with
        16- / 32- / 64-pixel packets (nrs_ctx_set_lane_teams)."""
        check(self.lib.nrs_ctx_set_lane_teams(self.h, int(lanes_per_ray)))

    def set_ray_handover(self, enabled):
        """Waves that run out of work take rays from a sibling wave of their workgroup (on by default; nrs_ctx_set_ray_handover)."""
        check(self.lib.nrs_ctx_set_ray_handover(self.h, int(bool(enabled))))

    def ray_handovers(self):
        """(rays moved, hand-overs) of the last render launch that returned statistics."""
        n, k = C.c_uint64(), C.c_uint64()
        check(self.lib.nrs_ctx_ray_handovers(self.h, C.byref(n), C.byref(k)))
        return n.value, k.value

    def render_launches(self):
        """(render-kernel dispatches enqueued through this context, schedule word of the last one) -- nrs_ctx_render_launches."""
        n, sched = C.c_uint64(), C.c_uint32()
        check(self.lib.nrs_ctx_render_launches(self.h, C.byref(n), C.byref(sched)))
        return n.value, sched.value
