"""CPU-only: the display step's entry points (nrs_tonemap, nrs_accumulate_spp_tonemap, nrs_tonemap_output_bytes) exist in the header, the ctypes mirror and the
library; the mirror of nrs_tonemap_params has the header's size; and every argument that no device is needed to judge is refused before a device is touched, with
its name in the message."""
import ctypes as C
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nrs_tonemap", "nrs_accumulate_spp_tonemap", "nrs_tonemap_output_bytes")


def test_tonemap_entry_points_are_exported(built):
    from nerfshop_amd import _abi
    lib = _abi.load()
    header = open(os.path.join(ROOT, "include", "nrs.h")).read()
    for name in NAMES:
        assert name in _abi.EXPORTS and hasattr(lib, name) and f"{name}(" in header
    assert "#define NRS_ABI_VERSION 3 " in header
    assert lib.nrs_abi_version() == 3   # appended exports: no layout changed
    assert f"#define NRS_TONEMAP_RGBA32F {_abi.TONEMAP_RGBA32F}u" in header and f"#define NRS_TONEMAP_RGBA8 {_abi.TONEMAP_RGBA8}u" in header


def test_mirror_has_the_size_of_the_header_struct(built, tmp_path):
    """sizeof and every field offset, printed by a C file compiled against include/nrs.h with the host compiler the examples are built with"""
    from nerfshop_amd import _abi
    fields = [f[0] for f in _abi.TonemapParams._fields_]
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include <nrs.h>\nint main(void) { printf("%zu", sizeof(nrs_tonemap_params));\n'
                   + "".join(f'printf(" %zu", offsetof(nrs_tonemap_params, {f}));\n' for f in fields) + "return 0; }\n")
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(_abi.TonemapParams) == 44
    assert got[1:] == [getattr(_abi.TonemapParams, f).offset for f in fields]
    assert _abi.TonemapParams().struct_size == got[0]


def test_output_bytes(built):
    from nerfshop_amd import _abi
    lib = _abi.load()
    for w, h in ((1, 1), (77, 53), (1920, 1080), (65536, 65535)):
        assert lib.nrs_tonemap_output_bytes(w, h, _abi.TONEMAP_RGBA32F) == 16 * w * h
        assert lib.nrs_tonemap_output_bytes(w, h, _abi.TONEMAP_RGBA8) == 4 * w * h
    assert lib.nrs_tonemap_output_bytes(4, 4, 2) == 0


def _params(**kw):
    from nerfshop_amd import _abi
    t = _abi.TonemapParams()
    for k, v in kw.items():
        setattr(t, k, v)
    return t


# (field values, a word of the message) of every params refusal
BAD_PARAMS = [
    ({"struct_size": 43}, b"struct_size"), ({"struct_size": 0}, b"struct_size"),
    ({"color_space": 3}, b"color_space"), ({"output_color_space": 2}, b"output_color_space"), ({"tonemap_curve": 4}, b"tonemap_curve"),
    ({"clamp_output": 2}, b"clamp_output"), ({"output_format": 2}, b"output_format"),
    ({"exposure": math.inf}, b"exposure"), ({"exposure": -math.inf}, b"exposure"), ({"exposure": math.nan}, b"exposure"),
]


def test_tonemap_arguments_refused_without_a_device(built):
    from nerfshop_amd import _abi
    lib = _abi.load()
    buf = (C.c_float * 16)()   # never dereferenced (nor is the "context"): every call below is refused first
    ptr = C.addressof(buf)
    other = ptr + 32
    W, H = 64, 36
    good = _params()

    def tonemap(ctx=ptr, w=W, h=H, acc=ptr, t=good, out=other):
        return lib.nrs_tonemap(ctx, None, w, h, acc, C.byref(t) if t is not None else None, out)

    def fused(ctx=ptr, w=W, h=H, frames=ptr, stride=W * H, K=2, acc=other, sc=0, t=good, out=other + 16):
        return lib.nrs_accumulate_spp_tonemap(ctx, None, w, h, frames, stride, K, acc, sc, C.byref(t) if t is not None else None, out)

    calls = [(lambda: tonemap(ctx=None), b"ctx"), (lambda: tonemap(acc=None), b"d_accumulate"), (lambda: tonemap(t=None), b"params"), (lambda: tonemap(out=None), b"d_out"),
             (lambda: tonemap(w=0), b"width"), (lambda: tonemap(h=0), b"height"),
             (lambda: fused(ctx=None), b"ctx"), (lambda: fused(frames=None), b"d_frames"), (lambda: fused(acc=None), b"d_accumulate"), (lambda: fused(t=None), b"params"),
             (lambda: fused(out=None), b"d_out"), (lambda: fused(w=0), b"width"), (lambda: fused(h=0), b"height"),
             # nrs_accumulate_spp's own
             (lambda: fused(K=0), b"spp_count"), (lambda: fused(K=_abi.SPP_BATCH_MAX + 1), b"NRS_SPP_BATCH_MAX"), (lambda: fused(stride=W * H - 1), b"slab_stride_pixels"),
             (lambda: fused(w=65536, h=65536, stride=1 << 40), b"too large"), (lambda: tonemap(w=65536, h=65536), b"too large")]
    for fields, word in BAD_PARAMS:
        calls.append((lambda f=fields: tonemap(t=_params(**f)), word))
        calls.append((lambda f=fields: fused(t=_params(**f)), word))
    for call, word in calls:
        assert call() == -1, word   # NRS_ERR_INVALID_ARG
        msg = lib.nrs_last_error()
        assert word in msg and msg.startswith(b"nrs_"), msg


@pytest.mark.parametrize("field,top", [("color_space", 2), ("output_color_space", 1), ("tonemap_curve", 3), ("clamp_output", 1), ("output_format", 1)])
def test_every_valid_value_passes_the_argument_check(built, field, top):
    """the refusals above are not a blanket 'no': with a NULL d_out behind valid params the complaint is about d_out, checked first, and with a valid d_out and a larger
    struct_size (a newer client) the params pass -- seen as the next refusal in line, the aliasing one, which needs no device either"""
    from nerfshop_amd import _abi
    lib = _abi.load()
    buf = (C.c_float * 16)()
    ptr = C.addressof(buf)
    for v in range(top + 1):
        t = _params(**{field: v})
        t.struct_size = C.sizeof(_abi.TonemapParams) + 8
        assert lib.nrs_accumulate_spp_tonemap(ptr, None, 4, 4, ptr, 16, 1, ptr + 16, 0, C.byref(t), ptr) == -1
        assert b"aliases" in lib.nrs_last_error(), lib.nrs_last_error()
