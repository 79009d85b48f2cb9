"""CPU-only: the entry points for several samples per pixel in one launch exist in the header, the ctypes mirror and the library, and refuse -- before they touch a
device -- the arguments that no device is needed to judge."""
import ctypes as C
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_spp_entry_points_are_exported(built):
    from nerfshop_amd import _abi
    lib = _abi.load()
    header = open(os.path.join(ROOT, "include", "nrs.h")).read()
    for name in ("nrs_render_nerf_spp", "nrs_accumulate_spp", "nrs_ctx_render_launches"):
        assert name in _abi.EXPORTS and hasattr(lib, name) and f"{name}(" in header
    assert f"#define NRS_SPP_BATCH_MAX {_abi.SPP_BATCH_MAX}u" in header
    assert lib.nrs_abi_version() == 3   # appended exports: no layout changed


def test_spp_arguments_refused_without_a_device(built):
    from nerfshop_amd import _abi
    lib = _abi.load()
    p = _abi.RenderParams()
    p.resolution[:] = (64, 36)
    buf = (C.c_float * 16)()   # never dereferenced: every call below is refused first
    ptr = C.addressof(buf)

    def render(K, frames=ptr, depths=ptr, model=None):
        return lib.nrs_render_nerf_spp(model, C.byref(p), None, 0, K, frames, depths, None, 64 * 36, None, None)

    for call, word in ((lambda: render(0), b"spp_count"), (lambda: render(_abi.SPP_BATCH_MAX + 1), b"NRS_SPP_BATCH_MAX"), (lambda: render(2, frames=None), b"d_frames"),
                       (lambda: render(2, depths=None), b"d_depths"), (lambda: render(2), b"NULL"), (lambda: render(1), b"NULL"),
                       (lambda: lib.nrs_accumulate_spp(None, None, 64, 36, ptr, 64 * 36, 2, ptr, 0, 0), b"NULL"),
                       (lambda: lib.nrs_ctx_render_launches(None, None, None), b"NULL")):
        assert call() == -1   # NRS_ERR_INVALID_ARG
        assert word in lib.nrs_last_error(), lib.nrs_last_error()
