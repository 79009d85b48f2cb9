"""The library's Makefile rebuilds what an edit touches and nothing else: header dependencies come from the compiler (the .d files beside the objects), one object
per subsystem, the render kernel's instantiations in shards of one source.  Dry runs only (`make -n -W <file>`: what WOULD be rebuilt if <file> were newer) -- nothing
is compiled.  Runs after build(); skipped where there is no make or no finished build to ask."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nerfshop_amd", "csrc")


def _rebuilt_if_touched(name):
    """Objects (without .o) that make would recompile, and whether it would link libnrs.so, if csrc/<name> were newer than everything."""
    if shutil.which("make") is None:
        pytest.skip("no make on this machine")
    deps = glob.glob(os.path.join(CSRC, "*.d"))
    if not deps or not all(os.path.exists(d[:-2] + ".o") for d in deps) or not os.path.exists(os.path.join(CSRC, "libnrs.so")):
        pytest.skip("no finished build beside the sources (.d files, their objects, libnrs.so): a dry run has nothing to compare with -- run build() first")
    assert os.path.exists(os.path.join(CSRC, name)), name
    up_to_date = subprocess.run(["make", "-n", "-C", CSRC], capture_output=True, text=True, check=True).stdout
    assert " -o " not in up_to_date, "the build is not up to date: a dry run says nothing about one file\n" + up_to_date
    out = subprocess.run(["make", "-n", "-W", name, "-C", CSRC], capture_output=True, text=True, check=True).stdout
    objects = set(re.findall(r" -o (\S+)\.o\b", out))
    return objects, re.search(r" -o libnrs\.so\b", out) is not None


# the units behind the C-ABI of include/nrs.h: what includes nrs_host.h
API_OBJECTS = {"nrs_api", "nrs_api_lowering", "nrs_api_model", "nrs_api_network", "nrs_api_edit", "nrs_api_render", "nrs_api_display"}


def _shards(objects):
    return {o for o in objects if o.startswith("nrs_render_rows_")}


def _all_shards():
    n = int(subprocess.run(["make", "-s", "-C", CSRC, "--eval", "print-shards: ; @echo $(ROW_SHARDS)", "print-shards"], capture_output=True, text=True, check=True).stdout)
    assert n >= 1
    return {f"nrs_render_rows_{k}" for k in range(n)}


def test_a_header_outside_any_hand_kept_list_reaches_its_includers():
    objects, link = _rebuilt_if_touched("nrs_svd3.h")
    assert objects == {"nrs_cage", "nrs_authoring"}, objects  # (and so neither the display object nor a render shard)
    assert link


def test_the_display_source_rebuilds_its_object_alone():
    objects, link = _rebuilt_if_touched("nrs_display.hip")
    assert objects == {"nrs_display"}, objects
    assert link


def test_the_render_kernel_header_rebuilds_every_shard_and_no_streaming_object():
    objects, link = _rebuilt_if_touched("nrs_render.cuh")
    assert _shards(objects) == _all_shards(), objects
    assert not objects & ({"nrs_display", "nrs_tables", "nrs_occupancy", "nrs_cage", "nrs_render"} | API_OBJECTS), objects
    # (slice_kernel takes the packet geometry from nrs_packets.cuh: the network object no longer sees the render kernel, and neither does any other subsystem)
    assert not objects & {"nrs_network", "nrs_network_backward", "nrs_train", "nrs_dataset", "nrs_mesh", "nrs_selection", "nrs_scan", "nrs_optimizer", "nrs_metrics"}, objects
    assert link


def test_the_edit_warp_header_rebuilds_every_shard_and_the_three_units_that_warp_samples():
    objects, link = _rebuilt_if_touched("nrs_edit_warp.cuh")
    assert _shards(objects) == _all_shards(), objects
    assert objects - _shards(objects) == {"nrs_cage", "nrs_occupancy", "nrs_tables"}, objects  # the users of the tet search and the affine warp outside the render kernel
    assert link


def test_the_mesh_launcher_header_rebuilds_the_mesh_unit_and_its_callers():
    objects, link = _rebuilt_if_touched("nrs_mesh.h")
    assert objects == {"nrs_mesh", "nrs_api_mesh"}, objects  # (no render shard, no other device object)
    assert link


def test_the_shade_header_reaches_no_unit_that_shades_nothing():
    objects, link = _rebuilt_if_touched("nrs_shade.cuh")
    assert not objects & {"nrs_cage", "nrs_selection", "nrs_tables", "nrs_scan", "nrs_optimizer", "nrs_metrics"}, objects
    assert link


def test_the_host_header_rebuilds_the_host_units_and_no_device_object():
    objects, link = _rebuilt_if_touched("nrs_host.h")
    assert objects == API_OBJECTS, objects  # (and so no device object, no render shard, none of the host units that stand alone)
    assert link
