"""The signed distance, what can be checked without a GPU: the checker itself (tests/sdf_ref.py) - the octahedron's known winding numbers, two overlapping cubes, points on
a vertex and in a face's plane, the reversed winding, and the float64 vector-Jacobian product of s against central differences - then the plumbing: the entry points are
declared, exported and listed, the ABI stays at 16, the unit is a row of the build ahead of `pointmesh`, and the entry points and the Python surface refuse wrong arguments
before they touch a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pointmesh_ref as pref
import sdf_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("psdr_hip_sdf_winding", "psdr_hip_sdf_grad")


@pytest.fixture(scope="module")
def psdr():
    import __graft_entry__
    __graft_entry__.build()
    import psdr_jit_amd
    return psdr_jit_amd


# ---- the checker

def test_octahedron_known_values():
    """the centre sees every face under 1 / 8 of the sphere; a far point sees nothing; the reversed mesh gives the negative"""
    v, f = ref.octahedron()
    th = ref.theta_matrix(np.zeros((1, 3)), v, f)
    assert np.abs(th / (2 * np.pi) - 0.125).max() <= 1e-15
    p = np.array([[0.0, 0.0, 0.0], [40.0, 30.0, -20.0], [0.2, -0.1, 0.3], [0.9, 0.8, 0.1]])
    w, G = ref.winding(p, v, f)
    assert np.abs(w - [1, 0, 1, 0]).max() <= 1e-14 and G[0] == pytest.approx(1.0, abs=1e-14) and (G >= np.abs(w) - 1e-15).all()
    assert ref.inside_of(w).tolist() == [True, False, True, False]
    wr, Gr = ref.winding(p, v, ref.reversed_faces(f))
    assert np.abs(wr + w).max() <= 1e-14 and np.abs(Gr - G).max() <= 1e-14
    assert ref.inside_of(wr, -1).tolist() == [True, False, True, False] and not ref.inside_of(wr, 1).any()
    w32, _g = ref.winding(p, v, f, np.float32)
    assert w32.dtype == np.float32 and np.abs(w32 - w).max() <= 16 * ref.U


def test_overlapping_cubes():
    v, f = ref.cubes()
    p = np.array([[0.75, 0.75, 0.75], [0.25, 0.25, 0.25], [1.25, 1.25, 1.25], [0.25, 1.25, 0.25], [-1.0, 0.5, 0.5]])
    w, _G = ref.winding(p, v, f)
    assert np.abs(w - [2, 1, 1, 0, 0]).max() <= 1e-14


def test_bunny_is_wound_counter_clockwise_and_nearly_closed():
    """a condition on the inputs of the GPU tests: orientation +1 is the bunny's, and its 42 boundary edges leave w within 0.05 of an integer well inside and outside"""
    v, f = pref.bunny()
    edges = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    _e, counts = np.unique(edges, axis=0, return_counts=True)
    assert (counts == 1).sum() == 42
    centre = (v.min(0) + v.max(0)).astype(np.float64) / 2
    w, _G = ref.winding(np.stack([centre, centre + 5.0]), v, f)
    assert abs(w[0] - 1) <= 0.05 and abs(w[1]) <= 0.05


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_points_on_a_vertex_and_in_a_plane_are_finite(dtype):
    """Nm == 0 is the principal value 0: a point on a vertex (a zero vector), a point in a face's plane, a face of zero area, a face over a repeated position - all pairs
    finite, and those contribute exactly 0"""
    v, f = ref.degenerate_mesh()
    p = np.concatenate([v, v[f[-2:]].mean(1), [[0.0, 5.0, 0.0]]]).astype(np.float32)
    th = ref.theta_matrix(p, v, f, dtype)
    assert np.isfinite(th).all()
    for i in range(len(v)):
        assert not th[i, (f == i).any(1)].any()                  # a vertex sees none of its own faces
    assert not th[:, -1].any()                                   # the face over a repeated position: b == c, the cross product is exactly 0
    plane = ref.theta(np.array([[3.0, -2.0, 0.0], [0.25, 0.25, 0.0]]), np.array([0.0, 0, 0]), np.array([1.0, 0, 0]), np.array([0.0, 1, 0]), dtype)
    assert not plane.any()                                       # in the plane z = 0, outside and inside the triangle
    w, G = ref.winding(p, v, f, dtype)
    assert np.isfinite(w).all() and np.isfinite(G).all()
    for name in ref.CASES:
        r = ref.reference(name)
        assert np.isfinite(r["w64"]).all() and np.isfinite(r["w32"]).all() and r["w32"].dtype == np.float32


def test_rule_has_room_on_the_named_cases():
    """the float32 checker against float64, in units of u: what the yardstick of the GPU rule is made of; and the condition of the sign test - at most 1 % of a closed case
    lies within the yardstick of 1 / 2"""
    for name in ref.CASES:
        for flipped in (False, True) if name in ("octahedron", "cubes") else (False,):
            r = ref.reference(name, flipped)
            e32, G = np.abs(r["w32"] - r["w64"]).max(), r["G"].max()
            yard = max(e32, ref.U * G)
            band = np.abs(np.abs(r["w64"]) - 0.5) <= yard
            print("%s%s: e_32 = %.1f u, G = %.2f, %d of %d points within the yardstick of 1 / 2" % (name, " reversed" if flipped else "", e32 / ref.U, G, band.sum(), len(band)))
            assert e32 <= 256 * ref.U * max(G, 1.0) and band.mean() <= 0.01


def test_vjp_against_central_differences():
    """float64, away from the medial axis and from the surface: the points are placed along the normals of the faces' centroids, at a distance well below the mesh's
    features, on both sides.  The indices and the sign are taken anew at every displaced input; the product with constant indices, barycentrics and sign equals the
    derivative of sum_i g_i s_i"""
    v32, f = ref.octahedron()
    r = np.random.default_rng(9)
    v = v32.astype(np.float64) * (0.9, 1.1, 0.7) + r.uniform(-0.02, 0.02, v32.shape)
    A, B, Cc = (v[f[:, k]] for k in range(3))
    n = np.cross(B - A, Cc - A)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    bary = r.dirichlet((4.0, 4.0, 4.0), len(f))
    q = bary[:, 0:1] * A + bary[:, 1:2] * B + bary[:, 2:3] * Cc
    p = np.concatenate([q + 0.07 * n, q - 0.05 * n])
    g = r.uniform(-1.0, 1.0, len(p))

    def value(p, v):
        c = pref.closest(p, v, f)
        w, _G = ref.winding(p, v, f)
        return c, ref.inside_of(w), float((g * ref.signed(c.dist2_p, ref.inside_of(w))).sum())

    c, inside, _total = value(p, v)
    assert inside.tolist() == [False] * len(f) + [True] * len(f) and (c.region_p == 7).all()
    s, gp, gv = ref.vjp(p, v, f, c.face_of_point, inside, g)
    assert np.allclose(s[:len(f)], 0.07, atol=1e-12) and np.allclose(s[len(f):], -0.05, atol=1e-12)
    h = 1e-6
    for which, grad in ((0, gp), (1, gv)):
        fd = np.zeros_like(grad)
        for i in range(grad.shape[0]):
            for k in range(3):
                vals = []
                for sgn in (+1, -1):
                    x = [p.copy(), v.copy()]
                    x[which][i, k] += sgn * h
                    vals.append(value(*x)[2])
                fd[i, k] = (vals[0] - vals[1]) / (2 * h)
        assert np.abs(grad).max() > 0.1 and np.abs(fd - grad).max() <= 2e-8 * max(np.abs(grad).max(), 1.0), (which, np.abs(fd - grad).max())
    # s == 0: both gradients are exactly 0
    s0, gp0, gv0 = ref.vjp(v, v, f, pref.closest(v, v, f).face_of_point, np.zeros(len(v), bool), np.ones(len(v)))
    assert not s0.any() and not gp0.any() and not gv0.any()
    f32 = ref.vjp(p.astype(np.float32), v.astype(np.float32), f, c.face_of_point, inside, g, np.float32)
    assert f32[2].dtype == np.float32 and np.abs(f32[2] - gv).max() <= 1e-4 * np.abs(gv).max()


# ---- the plumbing

def test_entry_points_declared_exported_listed(psdr):
    from psdr_jit_amd import build, cabi
    with open(os.path.join(ROOT, "include", "psdr_hip.h")) as fh:
        text = fh.read()
    L = cabi.lib()
    for name in NEW:
        assert re.search(r"^int\s+%s\s*\(" % name, text, re.M), "%s is not declared in include/psdr_hip.h" % name
        assert hasattr(L, name), "libpsdr_hip.so does not export %s" % name
        assert name in cabi.SYMBOLS
        assert getattr(L, name).argtypes is not None, "%s has no argtypes" % name
    assert text.index("THE POINT-TO-MESH DISTANCE") < text.index("THE SIGNED DISTANCE")
    assert re.search(r"#define\s+PSDR_HIP_ABI_VERSION\s+16\b", text) and L.psdr_hip_abi_version() == 16          # additive: the ABI stays at 16
    for name in ("SignedDistance", "SignedDistanceResult", "signed_distance", "winding_number"):
        assert hasattr(psdr, name)
    names = [u[0] for u in build.hip_units()]
    units = {u[0]: u for u in build.hip_units()}
    assert units["sdf"][1].endswith("sdf.hip") and units["sdf"][1] in build.HIP_SRCS
    assert names.count("sdf") == 1 and names.index("chamfer") < names.index("sdf") < names.index("pointmesh") and names[-1] == "pointmesh"
    deps = {os.path.relpath(d, ROOT) for d in units["sdf"][3]}
    assert {os.path.join("include", "psdr_hip.h"), os.path.join("psdr_jit_amd", "csrc", "hip", "mesh_pair.h"), os.path.join("psdr_jit_amd", "csrc", "hip", "nn_scan.h"), os.path.join("psdr_jit_amd", "csrc", "hip", "op_common.h"), os.path.join("psdr_jit_amd", "isa_lint.py")} <= deps
    contract = text[text.index("THE STREAM CONTRACT"):text.index("const char *psdr_hip_last_error")]
    assert all(name in contract for name in NEW)


def test_every_entry_point_refuses_bad_arguments_before_any_device_call(psdr):
    """no GPU is visible here: a call that reached the device would fail with a HIP error, not with the entry point's own message.  The non-NULL device pointers are host
    addresses that a refused call never reads."""
    from psdr_jit_amd import cabi
    L = cabi.lib()
    host = np.zeros(512, dtype=np.int64)
    p = [host.ctypes.data + 64 * i for i in range(30)]
    top = 1 << 26

    def refused(rc, name, word):
        msg = L.psdr_hip_last_error().decode()
        assert rc != 0 and msg.startswith(name + ":") and word in msg and "hip" not in msg[len(name):].lower(), (name, word, rc, msg)

    name = "psdr_hip_sdf_winding"
    keys = ("p", "v", "faces", "records", "partial", "dist2", "w", "sdf")

    def wind(N=4, n=4, F=4, orientation=1, **change):
        a = {k: p[i] for i, k in enumerate(keys)}
        a.update(change)
        return L.psdr_hip_sdf_winding(a["p"], N, a["v"], n, a["faces"], F, a["records"], a["partial"], a["dist2"], orientation, a["w"], a["sdf"], None)

    refused(wind(N=0), name, "n_points = 0")
    refused(wind(n=top + 1), name, "n_vertices = ")
    refused(wind(F=-2), name, "n_faces = -2")
    for bad in (0, 2, -3):
        refused(wind(orientation=bad), name, "orientation = %d" % bad)
    for key in ("p", "v", "faces", "records", "partial", "w"):
        refused(wind(**{key: None}), name, "NULL")
    refused(wind(dist2=None), name, "both")
    refused(wind(sdf=None), name, "both")

    name = "psdr_hip_sdf_grad"
    keys = ("p", "v", "faces", "face", "bary", "sdf", "g", "fb", "fl", "vb", "vc", "corners", "gp", "gv")

    def grad(N=4, n=4, F=4, **change):
        a = {k: p[i] for i, k in enumerate(keys)}
        a.update(change)
        return L.psdr_hip_sdf_grad(a["p"], N, a["v"], n, a["faces"], F, *[a[k] for k in keys[3:]], None)

    refused(grad(N=0), name, "n_points = 0")
    refused(grad(n=0), name, "n_vertices = 0")
    refused(grad(F=top + 1), name, "n_faces = ")
    for key in keys:
        refused(grad(**{key: None}), name, "NULL")
    refused(grad(gp=p[0]), name, "of their own")
    refused(grad(gv=p[1]), name, "of their own")
    refused(grad(gv=p[12]), name, "of their own")
    refused(grad(gp=p[6]), name, "of their own")
    assert not host.any()


def test_python_surface_refusals(psdr):
    """wrong arguments are a ValueError before a device is looked for (there is none here)"""
    import torch
    v, f = ref.octahedron()
    n = len(v)
    for orientation in (0, 2, -2, 1.0, 0.5, "1", None, True, (1,)):
        with pytest.raises(ValueError):
            psdr.SignedDistance(f, n, orientation=orientation)
        with pytest.raises(ValueError):
            psdr.signed_distance(torch.zeros(5, 3), torch.from_numpy(v), f, orientation=orientation)
    for args in ((f,), (f, 0), (f, 3), (f[:, :2], n), (f.astype(np.float64), n), (np.array([[0, 1, 1]]), 3), (np.zeros((0, 3), np.int64), 3)):
        with pytest.raises(ValueError):
            psdr.SignedDistance(*args)
    sd = psdr.SignedDistance(f, n)
    assert sd.orientation == 1 and sd.num_vertices == n and sd.winding is None and sd.nearest is None and psdr.SignedDistance(f, n, orientation=-1).orientation == -1
    mesh = type("M", (), {"face_indices": f.astype(np.int32), "num_vertices": n})()
    assert np.array_equal(psdr.SignedDistance(mesh).faces, f)
    good_p, good_v = torch.zeros(5, 3), torch.from_numpy(v)
    bad_points = (torch.zeros(5, 2), torch.zeros(0, 3), torch.zeros(5, 3, dtype=torch.int32), torch.zeros(5), torch.zeros(2, 5, 3), np.zeros((4, 3), np.int64))
    bad_vertices = (torch.zeros(n - 1, 3), torch.zeros(n, 2), torch.zeros(n, 3, dtype=torch.int64), torch.zeros(n))
    for args in [(bad, good_v) for bad in bad_points] + [(good_p, bad) for bad in bad_vertices]:
        with pytest.raises(ValueError):
            sd(*args)
        with pytest.raises(ValueError):
            sd.vjp(args[0], args[1], torch.zeros(5))
        with pytest.raises(ValueError):
            psdr.winding_number(args[0], args[1], f)
        with pytest.raises(ValueError):
            psdr.signed_distance(args[0], args[1], f)
    for bad in (f[:, :2], f.astype(np.float32), f + n, np.array([[0, 1, 1]]), np.zeros((0, 3), np.int64)):
        with pytest.raises(ValueError):
            psdr.winding_number(good_p, good_v, bad)
        with pytest.raises(ValueError):
            psdr.signed_distance(good_p, good_v, bad)
    for bad_g in (torch.zeros(4), torch.zeros(5, 1), torch.zeros(5, dtype=torch.int64)):
        with pytest.raises(ValueError):
            sd.vjp(good_p, good_v, bad_g)
    sd.orientation = 0                                        # the attribute is read at every call
    with pytest.raises(ValueError):
        sd(good_p, good_v)
    with pytest.raises(ValueError):
        sd.vjp(good_p, good_v, torch.zeros(5))
