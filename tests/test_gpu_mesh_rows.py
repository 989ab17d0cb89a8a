"""The device's mesh rows (psdr_mesh_geometry: k_geo_world / _face / _vnormal / _rows / _sec, csrc/hip/scene_build.hip) on the irregular corpus of
tests/mesh_rows_f64.py: open grids with holes, flat shading, a sheared transform with tangents on two factors, two moved meshes around an unmoved one, a 240-valence
fan, slivers with a zero-area face and an unused vertex, edges disabled, a textured mesh, coordinates around 1e4.  tests/test_mesh_rows_cpu.py holds the host's rows
against a float64 restatement of the reference; here every configure() after a move must give the host's rows bit for bit, a sound tree, the oracle's brute-force hits
bit for bit, and the images, derivatives and leaf gradients of a scene created from scratch in the same state.

And psdr_mesh_geometry's topology lists are validated before anything is filled or launched: one malformed list per check."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_rows_f64 as ref
import product

pytestmark = pytest.mark.gpu
CASES = ref.corpus()


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists)")
    import psdr_jit_amd as psdr
    from psdr_jit_amd import cabi
    return torch, psdr, cabi


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    oracle.build()
    return oracle


def _violations(cabi, sc):
    v = C.c_int64(-1)
    cabi.check(cabi.lib().psdr_hip_scene_check_tree(C.c_void_p(sc._hip_handle()), C.byref(v)))
    return v.value


def _trace(torch, cabi, sc, o, d):
    n = len(o)
    to, td = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    tri = torch.empty(n, dtype=torch.int32, device="cuda")
    uv = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    t = torch.empty(n, dtype=torch.float32, device="cuda")
    cabi.check(cabi.lib().psdr_hip_trace(sc._hip_handle(), n, to.data_ptr(), td.data_ptr(), tri.data_ptr(), uv.data_ptr(), t.data_ptr(), None))
    return tri.cpu().numpy(), uv.cpu().numpy(), t.cpu().numpy()


def _world(m):
    M = np.asarray(m.to_world_left, np.float64) @ np.asarray(m.to_world_raw, np.float64) @ np.asarray(m.to_world_right, np.float64)
    v = np.asarray(m.vertices, np.float64)
    return v @ M[:3, :3].T + M[:3, 3]


def _rays(spec, moved, seed):
    """from the camera: at every vertex and edge midpoint of the moved meshes (a hair off, both ways), and at random points of their boxes"""
    rng = np.random.default_rng(seed)
    cam = np.asarray(spec.cameras[0].to_world_raw, np.float64)[:3, 3]
    targets = []
    for i in moved:
        m = spec.meshes[i]
        V = _world(m)
        F = np.asarray(m.faces, np.int64)
        mid = 0.5 * (V[F] + V[np.roll(F, 1, axis=1)]).reshape(-1, 3)
        U = V[np.unique(F)]                                          # (not the unused vertex)
        span = U.max(axis=0) - U.min(axis=0) + 1e-3
        box = U.min(axis=0) + rng.uniform(size=(2000, 3)) * span
        targets += [V, V + 1e-4 * span * rng.standard_normal(V.shape), mid, mid + 1e-4 * span * rng.standard_normal(mid.shape), box]
    tg = np.concatenate(targets)
    d = tg - cam
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.broadcast_to(cam, d.shape)
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)


def _check_hits(torch, cabi, orc, sc, spec, moved, seed):
    o, d = _rays(spec, moved, seed)
    tri, uv, t = _trace(torch, cabi, sc, o, d)
    btri, buv, bt = orc.OracleScene(spec, [0]).trace(o, d, use_bvh=False)       # the definition: every triangle, smallest (t, id)
    assert np.array_equal(tri, btri)
    hit = btri >= 0
    assert hit.mean() > 0.3, hit.mean()
    assert np.array_equal(uv[hit], buv[hit]) and np.array_equal(t[hit], bt[hit])


def _same_image(a, b, tol=1e-6):
    """rel-L2 below tol, with the same non-finite pixels on both sides"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    fa, fb = np.isfinite(a), np.isfinite(b)
    assert np.array_equal(fa, fb)
    den = np.linalg.norm(b[fb])
    err = np.linalg.norm(a[fa] - b[fb]) / den if den > 0 else np.linalg.norm(a[fa])
    assert err < tol, err


def _tangent_row_bytes(spec):
    """the least the host path sends after a move or a new tangent: the tangent rows of every triangle (96 B; a move adds 144 B of traversal and shading rows)"""
    return 96 * sum(len(m.faces) for m in spec.meshes)


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_rows_on_irregular_meshes(env, orc, name):
    torch, psdr, cabi = env
    spec, moved = copy.deepcopy(CASES[name])
    sc, twin = product.build_scene(spec), product.build_scene(spec)
    assert sc._check_device_rows() == 0 and _violations(cabi, sc) == 0
    integ = psdr.PathTracer(2)
    for step in range(3):
        changes = ref.updates(spec, moved, step)
        ref.apply(sc, changes)
        sc.configure([0])
        info = sc._last_update()
        # the twin takes the same update through the host path (PSDR_HOST_GEOMETRY, read per call), which writes and sends every row
        ref.apply(twin, changes)
        os.environ["PSDR_HOST_GEOMETRY"] = "1"
        try:
            twin.configure([0])
        finally:
            del os.environ["PSDR_HOST_GEOMETRY"]
        host_bytes = twin._last_update()["bytes_uploaded"]
        assert host_bytes >= _tangent_row_bytes(spec) and twin._check_device_rows() == 0
        # the device computes the moved meshes' rows unless the layout changed - a tree built again (scene_sync: layout_same) - so that then the host's rows travel
        if info["tree"] == "built":
            assert info["bytes_uploaded"] >= 0.5 * host_bytes, (step, info, host_bytes)
        else:
            assert info["bytes_uploaded"] < 0.5 * host_bytes, (step, info, host_bytes)
        print(name, step, info["tree"], info["bytes_uploaded"], host_bytes)
        assert sc._check_device_rows() == 0, step
        assert _violations(cabi, sc) == 0, step
        _check_hits(torch, cabi, orc, sc, spec, moved, seed=step)
        fresh = product.build_scene(spec)
        img, dimg = psdr.render_d_fwd(integ, sc, 0, seed=30 + step)
        want, wd = psdr.render_d_fwd(integ, fresh, 0, seed=30 + step)
        _same_image(img.cpu().numpy(), want.cpu().numpy())
        _same_image(dimg.cpu().numpy(), wd.cpu().numpy())
        assert np.nanmax(np.abs(want.cpu().numpy())) > 0 and np.nanmax(np.abs(wd.cpu().numpy())) > 0
    # reverse mode: the leaf gradients of the updated scene = those of a scene made from scratch in the same state
    grads = []
    for s in (sc, product.build_scene(spec)):
        V = torch.tensor(np.asarray(spec.meshes[moved[0]].vertices), dtype=torch.float32).reshape(-1, 3).requires_grad_()
        s.param_map["Mesh[%d]" % moved[0]].vertex_positions = V
        s.configure([0])
        img = integ.renderD(s, 0, seed=41)
        w = torch.linspace(0.5, 1.5, img.numel(), device=img.device).reshape(img.shape)
        (img * w).sum().backward()
        grads.append(V.grad.cpu().numpy())
    _same_image(grads[0], grads[1])
    assert np.nanmax(np.abs(grads[1])) > 0


FAULTS = ["faces", "vf_begin[0]", "vf_begin order", "vf_begin end", "vf_item", "edges.v0", "edges.v1", "edges.opp", "edges.f0", "edges.f1"]
NAMED = {"faces": "faces", "vf_begin[0]": "vf_begin[0]", "vf_begin order": "vf_begin decreases", "vf_begin end": "vf_begin[n_vertices]", "vf_item": "vf_item",
         "edges.v0": "edges: v0", "edges.v1": "edges: v0", "edges.opp": "edges: v0", "edges.f0": "edges: f0", "edges.f1": "edges: f0"}


def test_malformed_geometry_is_refused_before_any_launch(env):
    """psdr_hip_scene_update with ONE malformed list of psdr_mesh_geometry (a new topology version, so that the lists are read): a non-zero return, the list named
    in psdr_hip_last_error(), and no kernel launched - the update carried the raw vertices scaled by 2, and the device's rows are still the host's rows of the
    unscaled state.  The configure() after each sends everything again and the scene is whole"""
    torch, psdr, cabi = env
    spec, moved = copy.deepcopy(CASES["three_meshes"])
    sc = product.build_scene(spec)
    ref.apply(sc, ref.updates(spec, moved, 0))
    sc.configure([0])                                              # (the device holds the topology of this version)
    assert sc._check_device_rows() == 0
    for fault in FAULTS:
        rc, msg = sc._update_with_malformed_geometry(2, fault)
        assert rc != 0 and "psdr_mesh_geometry[2]" in msg and NAMED[fault] in msg, (fault, rc, msg)
        assert sc._check_device_rows() == 0, fault
        sc.configure([0])                                          # (the failed update poisoned the handle: this one sends everything again)
        assert sc._check_device_rows() == 0 and _violations(cabi, sc) == 0, fault
    ref.apply(sc, ref.updates(spec, moved, 1))
    sc.configure([0])
    assert sc._check_device_rows() == 0 and _violations(cabi, sc) == 0
    img = psdr.PathTracer(2).renderC(sc, 0, seed=3).cpu().numpy()
    _same_image(img, psdr.PathTracer(2).renderC(product.build_scene(spec), 0, seed=3).cpu().numpy())
