"""Primary edges selected on the device (psdr_hip_scene_update_edges; the reference runs the silhouette test and compressD on device arrays in every Scene::configure,
src/sensor/perspective.cpp:52-151).  Bit equality is the definition of done: after every kind of update the device's edge arrays and both edge distributions are, word
for word, what the host path writes for the same state (psdr_hip_scene_check_edges), and the kept edges are those of a scene built from scratch on the host, in its order.

The scene: tests/scenes.py::config5_scene at level 3 - a 1280-face blob whose 1920 edges span several 256-thread workgroups (the cross-workgroup bases of the stable
compaction) - plus a flat-shaded 12-triangle cube (18 edges: less than one wave), an open two-triangle quad (boundary edges), a quad with a uv seam along its diagonal,
a mesh with enable_edges = False and a second sensor."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import product
import scenes

pytestmark = pytest.mark.gpu
BLOB_EDGES = 1920


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists)")
    import psdr_jit_amd as psdr
    return torch, psdr


@pytest.fixture(autouse=True)
def no_gate(monkeypatch):
    """the path is gated on an edge count (Scene::configure_host: below ~3840 edges the host loop is faster); the issue's test scene is smaller, so the tests lift the gate"""
    monkeypatch.setenv("PSDR_DEVICE_EDGES_MIN", "0")


def _cube(size):
    s = 0.5 * size
    v = np.asarray([[x, y, z] for x in (-s, s) for y in (-s, s) for z in (-s, s)], np.float32)          # index = 4 ix + 2 iy + iz
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]          # outward: -x +x -y +y -z +z
    f = np.asarray([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    return v, f


def _spec(sppe=2, sppse=2, extras=True):
    from oracle.oracle import CameraSpec, MeshSpec
    spec = scenes.config5_scene(48, 48, 2, sppe, sppse, level=3, env_res=(64, 32))
    assert len(spec.meshes[0].faces) == 1280
    if not extras:
        return spec
    v, f = _cube(60.0)
    cube = MeshSpec(vertices=v, faces=f, bsdf=1, use_face_normals=True)
    cube.to_world_raw = scenes.translate(60.0, 40.0, 120.0)
    quad_v = np.asarray([[0, 0, 0], [80, 0, 0], [80, 0, 80], [0, 0, 80]], np.float32)
    quad_f = np.asarray([[0, 2, 1], [0, 3, 2]], np.int32)
    quad = MeshSpec(vertices=quad_v, faces=quad_f, bsdf=1)                                                # open: four boundary edges, one coplanar inner edge
    quad.to_world_raw = scenes.translate(430.0, 60.0, 60.0)
    uv = np.asarray([[0, 0], [1, 0], [1, 1], [0, 0], [1, 1], [0, 1]], np.float32)
    seam = MeshSpec(vertices=quad_v.copy(), faces=quad_f.copy(), uvs=uv, face_uvs=np.asarray([[0, 2, 1], [3, 5, 4]], np.int32), bsdf=1)     # the faces share no uv index: a seam on the diagonal
    seam.to_world_raw = scenes.translate(430.0, 90.0, 200.0)
    off = MeshSpec(vertices=v.copy(), faces=f.copy(), bsdf=1, enable_edges=False)
    off.to_world_raw = scenes.translate(500.0, 40.0, 400.0)
    spec.meshes += [cube, quad, seam, off]
    spec.cameras.append(CameraSpec(50.0, 0.000001, 10000000.0, to_world_raw=scenes.translate(200.0, 300.0, -600.0) @ scenes._rot_x(np.radians(15.0))))
    return spec


def _check(sc, spec, active, step):
    """the device's words against the host path's, the kept edges against a scene built from scratch on the host in this state; -> kept edges of the blob per active sensor"""
    info = sc._last_update()
    assert info["edge_path"] == "device", (step, info)
    assert sc._check_device_edges() == 0, step
    fresh = product.build_scene(spec, host_only=True, active=active)
    kept = []
    for sid in range(len(spec.cameras)):
        name = "Sensor[%d]" % sid
        got = np.asarray(sc.param_map[name]._primary_edge_ids()).reshape(-1, 3)
        want = np.asarray(fresh.param_map[name]._primary_edge_ids()).reshape(-1, 3)
        assert np.array_equal(got, want), (step, sid, got.shape, want.shape)
        assert sc.param_map[name].enable_edges == fresh.param_map[name].enable_edges
        if sid in active:
            n = int((got[:, 0] == 0).sum())
            # (strictly between none and all: a kernel that keeps everything, or nothing, cannot pass for a compaction)
            assert 0 < n < BLOB_EDGES, (step, sid, n)
            kept.append(n)
    return kept


def test_the_device_selects_the_hosts_edges_bit_for_bit(env):
    torch, psdr = env
    spec = _spec()
    sc = product.build_scene(spec, active=(0, 1))
    assert sc._last_update()["edge_path"] == "host" and sc._check_device_edges() == 0           # (the create: the host's arrays)
    mesh, cube = sc.param_map["Mesh[0]"], sc.param_map["Mesh[2]"]
    v0 = np.asarray(spec.meshes[0].vertices, np.float32).copy()

    def move_vertices(scale_y):
        v = v0.copy(); v[:, 1] *= scale_y
        dv = np.zeros_like(v); dv[:, 2] = 0.5 * v[:, 0]
        mesh._set("vertex_positions", v, dv)
        spec.meshes[0].vertices, spec.meshes[0].d_vertices, spec.meshes[0].path = v, dv, None

    # the first update after the create gives the sensors' edge arrays their final size (the blob may move: the host's arrays once more) and leaves the world vertices on the device
    move_vertices(0.98)
    sc.configure([0, 1])
    assert sc._check_device_edges() == 0 and sc._check_device_rows() == 0
    # 1. a vertex move with a tangent
    move_vertices(0.93)
    sc.configure([0, 1])
    kept1 = _check(sc, spec, (0, 1), "vertices")
    assert sc._check_device_rows() == 0
    # 2. a to_world_left change with a tangent (the flat-shaded cube: 18 edges, less than one wave)
    t = np.eye(4, dtype=np.float32); t[0, 3] = 25.0; t[1, 3] = 10.0
    dT = np.zeros((4, 4), np.float32); dT[0, 3] = 100.0
    cube._set("to_world_left", t, dT)
    spec.meshes[2].to_world_left, spec.meshes[2].d_to_world_left = t, dT
    sc.configure([0, 1])
    _check(sc, spec, (0, 1), "to_world_left")
    # 3. a camera-only move with a tangent on Sensor.to_world: no geometry work, no edge arrays from the host
    cam0 = sc.param_map["Sensor[0]"]
    c = (scenes.translate(330.0, 420.0, -650.0) @ scenes._rot_x(np.radians(27.0))).astype(np.float32)
    dC = np.zeros((4, 4), np.float32); dC[0, 3] = 50.0
    cam0._set("to_world", c, dC)
    spec.cameras[0].to_world_raw, spec.cameras[0].d_to_world_raw = c, dC
    sc.configure([0, 1])
    kept3 = _check(sc, spec, (0, 1), "camera")
    assert sc._last_update()["tree"] == "kept"
    assert kept3[1] == kept1[1]                                      # (the second sensor did not move: it keeps the selection it had)
    # 4. configure([1]): the second sensor alone, after a move of its own
    cam1 = sc.param_map["Sensor[1]"]
    c1 = (scenes.translate(180.0, 330.0, -560.0) @ scenes._rot_x(np.radians(18.0))).astype(np.float32)
    cam1._set("to_world", c1, dC)
    spec.cameras[1].to_world_raw, spec.cameras[1].d_to_world_raw = c1, dC
    sc.configure([1])
    _check(sc, spec, (1,), "second sensor")
    # the host's copy on demand is the device's selection (Scene::ensure_host_edges refuses another one)
    rows = np.asarray(sc.param_map["Sensor[1]"]._primary_edges(False))
    fresh = product.build_scene(spec, host_only=True, active=(1,))
    assert np.array_equal(rows, np.asarray(fresh.param_map["Sensor[1]"]._primary_edges(False)))
    assert np.array_equal(np.asarray(sc.param_map["Sensor[1]"]._primary_edges(True)), np.asarray(fresh.param_map["Sensor[1]"]._primary_edges(True)))


def _warm(sc, spec, active=(0,)):
    """two vertex moves: the first update after the create sizes the edge arrays (and may move the blob), from the second on the device selects"""
    mesh = sc.param_map["Mesh[0]"]
    v0 = np.asarray(spec.meshes[0].vertices, np.float32)
    for k in (0.99, 0.97):
        v = v0.copy(); v[:, 1] *= k
        mesh._set("vertex_positions", v, np.zeros_like(v))
        sc.configure(list(active))
    spec.meshes[0].vertices, spec.meshes[0].d_vertices = v, None
    return v


def test_the_scan_is_used_where_it_is_exact_and_the_sequential_form_elsewhere(env):
    """the cmf is DiscreteDistribution::init's sequential double running sum: a parallel scan only where every partial sum is exact in double (checked on the device) - the
    test scene's lengths qualify; a speck of 1e-4 among edges of 560 spreads the exponents of the secondary edges too far and one lane runs the sequential form.  Same bits."""
    from oracle.oracle import MeshSpec
    torch, psdr = env
    spec = _spec()
    sc = product.build_scene(spec)
    _warm(sc, spec)
    info = sc._last_update()
    assert info["edge_path"] == "device" and info["edge_cdf"] == "scan", info
    assert sc._check_device_edges() == 0
    spec = _spec()
    speck = MeshSpec(vertices=np.asarray([[0, 0, 0], [1e-4, 0, 0], [1e-4, 0, 1e-4], [0, 0, 1e-4]], np.float32), faces=np.asarray([[0, 2, 1], [0, 3, 2]], np.int32), bsdf=1)
    spec.meshes.append(speck)
    sc = product.build_scene(spec)
    _warm(sc, spec)
    info = sc._last_update()
    assert info["edge_path"] == "device" and info["edge_cdf"] == "sequential", info
    assert sc._check_device_edges() == 0 and sc._check_device_rows() == 0


@pytest.mark.parametrize("sppe,sppse", [(0, 2), (2, 0)])
def test_scenes_without_one_of_the_edge_terms(env, sppe, sppse):
    """sppe = 0: no sensor has primary edges, the secondary-edge distribution is still the device's; sppse = 0: no secondary edges, the primary ones are selected on the device"""
    torch, psdr = env
    spec = _spec(sppe, sppse)
    sc = product.build_scene(spec)
    _warm(sc, spec)
    info = sc._last_update()
    assert info["edge_path"] == "device", info
    assert sc._check_device_edges() == 0 and sc._check_device_rows() == 0
    ids = np.asarray(sc.param_map["Sensor[0]"]._primary_edge_ids()).reshape(-1, 3)
    fresh = product.build_scene(spec, host_only=True)
    assert np.array_equal(ids, np.asarray(fresh.param_map["Sensor[0]"]._primary_edge_ids()).reshape(-1, 3))
    assert (len(ids) > 0) == (sppe > 0) and sc.param_map["Sensor[0]"].enable_edges == (sppe > 0)
    img, dimg = psdr.render_d_fwd(psdr.PathTracer(2), sc, 0, seed=3)
    assert np.isfinite(img.cpu().numpy()).all() and np.isfinite(dimg.cpu().numpy()).all()


def test_a_mesh_that_keeps_no_edge_raises_as_on_the_host_and_the_scene_recovers(env):
    """the reference asserts slices(info) > 0 per mesh (perspective.cpp:112-118): a camera inside the closed flat-shaded cube sees only back faces, the cube keeps no edge.  The host
    loop raises in the middle of configure(); with the selection on the device the count comes back after the upload and the same PsdrException text is raised; once the camera has
    moved out again configure() works and the device holds the host's bits"""
    torch, psdr = env
    spec = _spec()
    sc = product.build_scene(spec)
    _warm(sc, spec)
    assert sc._last_update()["edge_path"] == "device"
    cam = sc.param_map["Sensor[0]"]
    outside = np.asarray(spec.cameras[0].to_world_raw, np.float32)
    inside = scenes.translate(60.0, 40.0, 120.0)
    zero = np.zeros((4, 4), np.float32)
    cam._set("to_world", inside, zero)
    with pytest.raises(RuntimeError, match=r"slices\(info\) > 0"):
        sc.configure([0])
    spec.cameras[0].to_world_raw = inside
    with pytest.raises(RuntimeError, match=r"slices\(info\) > 0"):            # (the host path in the same state)
        product.build_scene(spec, host_only=True)
    moved_out = (scenes.translate(0.0, 10.0, 0.0) @ outside).astype(np.float32)
    cam._set("to_world", moved_out, zero)
    spec.cameras[0].to_world_raw = moved_out
    sc.configure([0])
    _check(sc, spec, (0,), "recovered")


def test_what_no_longer_travels(env, monkeypatch):
    """bytes, derived: per kept primary edge the host path sends p0, p1, d_p0, d_p1 and normal at 8 B each and length, pmf and cmf at 4 B each = 52 B, per secondary edge pmf and
    cmf = 8 B; the device path sends none of them - after a vertex move the raw vertices and their tangents (24 B per vertex of the moved mesh) and the small tables travel, after
    a camera-only move no edge bytes at all"""
    torch, psdr = env
    spec = _spec()
    sc = product.build_scene(spec)
    v = _warm(sc, spec)
    mesh, cam = sc.param_map["Mesh[0]"], sc.param_map["Sensor[0]"]

    def move(scene, k):
        w = v.copy(); w[:, 0] *= k
        scene.param_map["Mesh[0]"]._set("vertex_positions", w, np.zeros_like(w))
        scene.configure([0])
        return scene._last_update()

    dev = move(sc, 0.96)
    assert dev["edge_path"] == "device" and dev["edge_bytes"] == 0, dev
    kept = len(np.asarray(cam._primary_edge_ids()).reshape(-1, 3))
    n_sec = sum(m.num_edges() for m in (sc.param_map["Mesh[%d]" % i] for i in range(len(spec.meshes))) if m.enable_edges)
    assert kept > 0 and n_sec >= BLOB_EDGES
    assert dev["bytes_uploaded"] <= 24 * len(v) + 8192, dev
    # the same update through the host path
    monkeypatch.setenv("PSDR_HOST_GEOMETRY", "1")
    host = move(sc, 0.95)
    monkeypatch.delenv("PSDR_HOST_GEOMETRY")
    assert host["edge_path"] == "host" and sc._check_device_edges() == 0
    kept_host = len(np.asarray(cam._primary_edge_ids()).reshape(-1, 3))
    # what the host path sends FOR THE EDGES (its other bytes are triangle rows): at least the 52 B per kept primary edge and the 8 B per secondary edge the device path saves
    assert host["edge_bytes"] >= 52 * kept_host + 8 * n_sec, (host, kept_host, n_sec)
    again = move(sc, 0.96)                      # (the state of `dev` once more, through the device path)
    assert again["edge_bytes"] == 0 and host["bytes_uploaded"] - again["bytes_uploaded"] >= 52 * kept + 8 * n_sec, (host, again, kept, n_sec)
    # a camera-only configure sends no edge bytes at all
    move(sc, 0.97)
    c = (scenes.translate(5.0, 0.0, 0.0) @ np.asarray(spec.cameras[0].to_world_raw, np.float32)).astype(np.float32)
    cam._set("to_world", c, np.zeros((4, 4), np.float32))
    sc.configure([0])
    info = sc._last_update()
    assert info["edge_path"] == "device" and info["edge_bytes"] == 0 and info["tree"] == "kept", info
    assert info["bytes_uploaded"] < 8192, info
    assert sc._check_device_edges() == 0


def test_rendering_through_the_device_path_equals_the_host_path(env, monkeypatch):
    """renderD, forward_grad and loss.backward() into the vertices and the camera pose: the same state through the device selection and forced through the host path
    (PSDR_HOST_GEOMETRY=1) - the inputs of the kernels are the same bits, so the tolerance is the one of tests/test_gpu_configure.py for same-state comparisons"""
    torch, psdr = env

    def run(host):
        if host:
            monkeypatch.setenv("PSDR_HOST_GEOMETRY", "1")
        spec = _spec()
        sc = product.build_scene(spec)
        _warm(sc, spec)
        mesh, cam = sc.param_map["Mesh[0]"], sc.param_map["Sensor[0]"]
        gen = torch.Generator().manual_seed(0)
        V = torch.tensor(np.asarray(spec.meshes[0].vertices, np.float32) * np.asarray([1.0, 0.9, 1.0], np.float32), requires_grad=True)
        C = psdr.FloatD(0.1).requires_grad_()
        base = torch.tensor(np.asarray(spec.cameras[0].to_world_raw, np.float32))
        shift = torch.zeros(4, 4); shift[0, 3] = 1.0
        mesh.vertex_positions = V
        cam.to_world = psdr.Matrix4fD(base + shift * C * 50.)
        sc.configure([0])
        path = sc._last_update()["edge_path"]
        img = psdr.PathTracer(2).renderD(sc, 0, seed=4)
        w = (torch.rand(img.shape, generator=gen) + 0.5).to(img.device)
        dV = torch.randn(V.shape, generator=gen)
        d_C = psdr.forward_grad(img, C).detach().cpu().numpy()
        d_V = psdr.forward_grad(img, V, direction=dV).detach().cpu().numpy()
        (img * w).sum().backward()
        out = {"img": img.detach().cpu().numpy(), "d_C": d_C, "d_V": d_V, "g_V": V.grad.detach().cpu().numpy(), "g_C": np.asarray([float(C.grad)])}
        if host:
            monkeypatch.delenv("PSDR_HOST_GEOMETRY")
        return path, out

    path_d, dev = run(False)
    path_h, host = run(True)
    assert path_d == "device" and path_h == "host"
    for k in dev:
        assert np.abs(host[k]).max() > 0, k
        err = product.rel_l2(dev[k], host[k])
        print(k, err)
        assert err < 1e-6, (k, err)


def test_the_gate_and_a_scene_large_enough_for_the_search_tables(env, monkeypatch):
    """without the test knob: the 1920-edge scene stays with the host loop (measured slower on the device), the blob at level 5 (30 720 edges, thousands kept: both distributions get
    a search table, built on the device and compared entry by entry by the check) takes the device path"""
    torch, psdr = env
    monkeypatch.delenv("PSDR_DEVICE_EDGES_MIN")
    spec = _spec()
    sc = product.build_scene(spec)
    _warm(sc, spec)
    info = sc._last_update()
    assert info["edge_path"] == "host" and info["edge_bytes"] > 0, info
    assert sc._check_device_edges() == 0 and sc._check_device_rows() == 0
    spec = scenes.config5_scene(48, 48, 2, 2, 2, level=5, env_res=(64, 32))
    sc = product.build_scene(spec)
    _warm(sc, spec)
    info = sc._last_update()
    assert info["edge_path"] == "device" and info["edge_bytes"] == 0, info
    kept = len(np.asarray(sc.param_map["Sensor[0]"]._primary_edge_ids()).reshape(-1, 3))
    assert 256 <= kept < 30720, kept
    assert sc._check_device_edges() == 0 and sc._check_device_rows() == 0
    fresh = product.build_scene(spec, host_only=True)
    assert np.array_equal(np.asarray(sc.param_map["Sensor[0]"]._primary_edge_ids()), np.asarray(fresh.param_map["Sensor[0]"]._primary_edge_ids()))
