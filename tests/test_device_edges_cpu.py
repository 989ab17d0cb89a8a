"""Primary edges selected on the device (psdr_hip_scene_update_edges): what can be checked without a GPU - the new entry points are declared in the header,
exported by the library and listed in the ctypes view, the ABI version and the structs did not move, and the keep test and the row both sides compile
(psdr_jit_amd/csrc/host/edge_select.h) give the values written in tests/cpp/edge_select_check.cpp on hand-made edges: silhouette, crease, coplanar, boundary,
uv seam.  That the host loop, which now calls the same functions, still writes the bits it wrote before is what tests/test_host_cpu.py pins."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("psdr_hip_scene_update_edges", "psdr_hip_scene_primary_edges", "psdr_hip_scene_check_edges", "psdr_hip_scene_edge_path")


@pytest.fixture(scope="module")
def psdr():
    import __graft_entry__
    __graft_entry__.build()
    import psdr_jit_amd
    return psdr_jit_amd


def _header():
    with open(os.path.join(ROOT, "include", "psdr_hip.h")) as fh:
        return fh.read()


def test_edge_entry_points_declared_exported_listed(psdr):
    from psdr_jit_amd import cabi
    text = _header()
    L = cabi.lib()
    for name in NEW:
        assert re.search(r"^int\s+%s\s*\(" % name, text, re.M), "%s is not declared in include/psdr_hip.h" % name
        assert hasattr(L, name), "libpsdr_hip.so does not export %s" % name
        assert name in cabi.SYMBOLS
    assert re.search(r"typedef struct psdr_edge_topology \{", text)
    for mode, value in (("HOST", 0), ("DEVICE", 1), ("KEEP", 2)):
        assert re.search(r"#define\s+PSDR_EDGES_%s\s+%d\b" % (mode, value), text)
    # the comment that conceded the sensors' primary edges to the host is gone
    assert "the sensors' primary edges still come from the host" not in text


def test_abi_version_and_structs_did_not_move(psdr):
    from psdr_jit_amd import cabi
    text = _header()
    assert re.search(r"#define\s+PSDR_HIP_ABI_VERSION\s+16\b", text)
    assert cabi.lib().psdr_hip_abi_version() == 16
    assert [f[0] for f in cabi.RenderArgs._fields_][-2:] == ["skip_static_edges", "shard_mode"]
    assert [f[0] for f in cabi.UpdateInfo._fields_] == ["tree", "reallocated", "bytes_uploaded", "sah_cost", "sah_cost_built", "ms_tree", "ms_fill", "ms_upload", "ms_total"]
    # the structs the update reads end where they ended: the new call takes what it needs as arguments of its own
    def last_member(name):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return re.findall(r"(\w+)\s*;", body)[-1]
    assert last_member("psdr_scene_snapshot") == "rows_valid"
    assert last_member("psdr_sensor_rec") == "edge_sum"
    assert last_member("psdr_mesh_geometry") == "moved"
    assert last_member("psdr_update_info") == "ms_total"


def test_null_arguments_are_refused_before_any_device_call(psdr):
    from psdr_jit_amd import cabi
    L = cabi.lib()
    n, s = C.c_int32(-1), C.c_int64(-1)
    assert L.psdr_hip_scene_update_edges(None, None, 0, None, None, None) != 0
    assert L.psdr_hip_scene_primary_edges(None, 0, C.byref(n), None, 0, None) != 0
    assert L.psdr_hip_scene_check_edges(None, None, C.byref(s)) != 0
    assert L.psdr_hip_scene_edge_path(None, C.byref(n), C.byref(s)) != 0


def test_shared_keep_test_and_row_on_hand_made_edges(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "edge_select_check.cpp")
    exe = os.path.join(tmp_path, "edge_select_check")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-I" + ROOT, src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout[-2000:]


def test_the_chosen_scene_keeps_some_but_not_all_edges_on_the_host(psdr):
    """what the GPU tests rely on (tests/test_gpu_device_edges.py): on the host path alone the blob of their scene keeps strictly between none and all of its 1920
    edges, so a kernel that keeps everything or nothing cannot pass for a compaction"""
    import product
    import scenes
    spec = scenes.config5_scene(48, 48, 2, 2, 2, level=3, env_res=(64, 32))
    assert len(spec.meshes[0].faces) == 1280
    sc = product.build_scene(spec, host_only=True)
    ids = np.asarray(sc.param_map["Sensor[0]"]._primary_edge_ids()).reshape(-1, 3)
    assert sc.param_map["Mesh[0]"].num_edges() == 1920
    kept = int((ids[:, 0] == 0).sum())
    assert 0 < kept < 1920, kept
    # the host's uv-seam byte per edge exists only for meshes with uv coordinates; its selection is in mesh order
    assert (np.diff(ids[:, 0]) >= 0).all()
