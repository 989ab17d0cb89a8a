"""Marching tetrahedra, what can be checked without a GPU: the checker itself (tests/mtet_ref.py) - all 256 sign patterns of one cell, a sphere that must come out closed,
consistently oriented, of Euler characteristic 2 and of positive volume, and the float64 vector-Jacobian product against central differences - then the plumbing: the entry
points are declared, exported and listed, the ABI stays at 16, the unit is the one row of its list between `sdf` and `pointmesh`, the plan of the Python layer is the library's,
and the entry points and the Python surface refuse wrong arguments before they touch a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mtet_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("psdr_hip_mtet_plan", "psdr_hip_mtet_count", "psdr_hip_mtet_emit", "psdr_hip_mtet_vertices", "psdr_hip_mtet_vertices_adj")


@pytest.fixture(scope="module")
def psdr():
    import __graft_entry__
    __graft_entry__.build()
    import psdr_jit_amd
    return psdr_jit_amd


# ---- the checker

def test_tets_and_slots_of_one_cell():
    """six tetrahedra from corner 0 to corner 7, every one of volume 1 / 6, together the 19 edges of the seven classes: 12 cube edges, 6 face diagonals, the body diagonal"""
    shape = (2, 2, 2)
    T = ref.tets(shape)
    assert T.shape == (6, 4) and (T[:, 0] == 0).all() and (T[:, 3] == 7).all() and T[0].tolist() == [0, 1, 3, 7] and T[5].tolist() == [0, 4, 6, 7]
    X = ref.coords(shape).astype(np.float64)
    vol = np.abs(np.linalg.det(X[T[:, 1:]] - X[T[:, :1]])) / 6
    assert np.allclose(vol, 1 / 6)
    edges = {(int(t[i]), int(t[j])) for t in T for i in range(4) for j in range(i + 1, 4)}
    assert len(edges) == 19 and all(a < b for a, b in edges)
    slots, ends = ref.crossing_slots(shape, np.arange(8) == 0)          # corner 0 alone inside: its seven slots cross
    assert slots.tolist() == list(range(7)) and ends[:, 0].tolist() == [0] * 7 and ends[:, 1].tolist() == [1, 2, 4, 3, 5, 6, 7]


def test_one_cell_all_256_patterns():
    """every undirected mesh edge that does not lie in a face of the cube is used by exactly two triangles, in opposite directions; every triangle's normal points from its
    tetrahedron's inside corners to its outside corners; patterns 0 and 255 give nothing"""
    shape = (2, 2, 2)
    X = ref.coords(shape).astype(np.float64)
    T = ref.tets(shape)
    total = 0
    for pattern in range(256):
        sdf = np.where(pattern >> np.arange(8) & 1, -1.0, 1.0).astype(np.float32)
        r = ref.topology(sdf, shape)
        if pattern in (0, 255):
            assert len(r["edges"]) == 0 and len(r["faces"]) == 0
            continue
        assert len(r["faces"]) > 0 and len(r["edges"]) > 0 and np.array_equal(np.unique(r["faces"]), np.arange(len(r["edges"])))
        v = ref.positions(sdf, X, r["edges"])
        assert np.array_equal(v, (X[r["edges"][:, 0]] + X[r["edges"][:, 1]]) / 2)
        dc = ref.directed_edge_counts(r["faces"])
        for (i, j), k in dc.items():
            in_a_face = (((v[i] == 0) & (v[j] == 0)) | ((v[i] == 1) & (v[j] == 1))).any()
            if in_a_face:
                assert k == 1 and (j, i) not in dc, (pattern, i, j)
            else:
                assert k == 1 and dc.get((j, i)) == 1, (pattern, i, j)
        f = r["faces"]
        normal = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
        ins = ref.inside(sdf)[T[r["face_tet"]]]
        corners = X[T[r["face_tet"]]]
        to_outside = (corners * ~ins[:, :, None]).sum(1) / (~ins).sum(1)[:, None] - (corners * ins[:, :, None]).sum(1) / ins.sum(1)[:, None]
        assert ((normal * to_outside).sum(1) > 0).all(), pattern
        assert (np.diff(r["face_tet"]) >= 0).all()
        total += len(f)
    assert total > 0


def test_sphere_is_a_closed_oriented_surface():
    shape = ref.SPHERE_SHAPE
    pos, sdf = ref.sphere()
    assert shape == (12, 11, 10) and np.abs(sdf).min() >= 1e-3          # the condition on the input: no lattice vertex in a band around the surface
    r = ref.reference(sdf, pos, shape, key="sphere")
    V, F = len(r["edges"]), len(r["faces"])
    assert V > 100 and ref.closed_and_oriented(r["faces"])
    assert ref.euler(r["faces"], V) == 2
    vol = ref.signed_volume(r["v64"], r["faces"])
    assert 0.8 * 4 / 3 * np.pi * ref.SPHERE_RADIUS ** 3 < vol < 4 / 3 * np.pi * ref.SPHERE_RADIUS ** 3          # positive: counter-clockwise seen from outside; inscribed
    assert np.abs(np.linalg.norm(r["v64"] - ref.SPHERE_CENTRE, axis=1) - ref.SPHERE_RADIUS).max() < ref.cell_diagonal(shape)
    assert np.abs(r["v32"] - r["v64"]).max() <= 8 * ref.U


def test_zero_and_nan_are_outside_and_coincident_vertices_are_kept():
    shape = (5, 3, 3)
    X = ref.coords(shape)
    sdf = (X[:, 0] - 2).astype(np.float32)                              # zeros on the whole plane x = 2
    r = ref.reference(sdf, X.astype(np.float32), shape)
    assert np.array_equal(ref.inside(sdf), X[:, 0] < 2)
    assert (ref.coords(shape, r["edges"][:, 0])[:, 0] == 1).all() and (ref.coords(shape, r["edges"][:, 1])[:, 0] == 2).all()
    assert np.isfinite(r["v32"]).all() and (r["v32"][:, 0] == 2).all()                                # t = 1: the far end
    assert len(np.unique(r["v32"], axis=0)) < len(r["v32"])                                           # several slots coincide
    nan = sdf.copy()
    nan[X[:, 0] >= 2] = np.nan
    assert np.array_equal(ref.topology(nan, shape)["faces"], r["faces"]) and np.array_equal(ref.topology(nan, shape)["edges"], r["edges"])


def test_vjp_against_central_differences():
    """float64, at fixed topology: the values are kept away from zero so that no displaced input changes a sign"""
    shape = (3, 4, 3)
    sdf = ref.random_sdf(shape, 5, keep_away=0.2).astype(np.float64)
    pos = ref.jittered(shape, 6).astype(np.float64)
    r = ref.topology(sdf, shape)
    edges = r["edges"]
    g = np.random.default_rng(7).uniform(-1, 1, (len(edges), 3))
    gs, gp = ref.vjp(sdf, pos, edges, g, shape)
    value = lambda s, p: float((g * ref.positions(s, p, edges)).sum())
    h = 1e-6
    fd_s, fd_p = np.zeros_like(gs), np.zeros_like(gp)
    for u in range(len(sdf)):
        for sgn in (1, -1):
            s = sdf.copy()
            s[u] += sgn * h
            assert np.array_equal(ref.inside(s), ref.inside(sdf))
            fd_s[u] += sgn * value(s, pos) / (2 * h)
            for k in range(3):
                p = pos.copy()
                p[u, k] += sgn * h
                fd_p[u, k] += sgn * value(sdf, p) / (2 * h)
    assert np.abs(gs).max() > 0.1 and np.abs(gp).max() > 0.1
    assert np.abs(fd_s - gs).max() <= 1e-7 * max(np.abs(gs).max(), 1.0), np.abs(fd_s - gs).max()
    assert np.abs(fd_p - gp).max() <= 1e-7 * max(np.abs(gp).max(), 1.0), np.abs(fd_p - gp).max()
    gs32, gp32 = ref.vjp(sdf, pos, edges, g, shape, np.float32)
    assert gs32.dtype == np.float32 and np.abs(gs32 - gs).max() <= 1e-4 * np.abs(gs).max() and np.abs(gp32 - gp).max() <= 1e-5 * np.abs(gp).max()


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
    assert text.index("THE SIGNED DISTANCE") < text.index("THE ISOSURFACE")
    assert re.search(r"#define\s+PSDR_HIP_ABI_VERSION\s+16\b", text) and L.psdr_hip_abi_version() == 16          # additive: the ABI stays at 16
    for name in ("MarchingTetrahedra", "MtetTopology", "lattice_points", "launch_plan_mt"):
        assert hasattr(psdr, name)
    names = [u[0] for u in build.hip_units()]
    units = {u[0]: u for u in build.hip_units()}
    assert units["mtet"][1].endswith("mtet.hip") and units["mtet"][1] in build.HIP_SRCS
    assert names.count("mtet") == 1 and names.index("sdf") < names.index("mtet") < names.index("pointmesh") and names[-1] == "pointmesh"
    deps = {os.path.relpath(d, ROOT) for d in units["mtet"][3]}
    assert {os.path.join("include", "psdr_hip.h"), os.path.join("psdr_jit_amd", "csrc", "hip", "op_common.h"), os.path.join("psdr_jit_amd", "isa_lint.py")} <= deps
    contract = text[text.index("THE STREAM CONTRACT"):text.index("const char *psdr_hip_last_error")]
    assert all(name in contract for name in NEW)


def test_plan_of_the_python_layer_is_the_librarys(psdr):
    from psdr_jit_amd import cabi
    L = cabi.lib()
    for shape in ((2, 2, 2), (8, 4, 2), (8, 4, 3), (16, 16, 2), (17, 17, 2), (33, 33, 33), (256, 128, 2), (256, 129, 2), (257, 257, 2), (257, 258, 2), (256, 256, 256)):
        out = [C.c_int32() for _ in range(6)]
        assert L.psdr_hip_mtet_plan(*shape, *[C.byref(o) for o in out]) == 0
        p = psdr.launch_plan_mt(shape)
        assert [o.value for o in out] == [p.tile, p.vertex_blocks, p.cell_blocks, p.vertex_passes, p.cell_passes, p.scratch_ints], shape
        assert (p.num_lattice, p.num_cells) == ref.counts(shape) and p.wave == 64
    p = psdr.launch_plan_mt((256, 256, 256))
    assert p.num_lattice == 1 << 24 and p.vertex_blocks == p.tile ** 2 and p.vertex_passes == 2          # the largest lattice needs no third pass
    assert psdr.launch_plan_mt((256, 128, 2)).vertex_passes == 1 and psdr.launch_plan_mt((256, 129, 2)).vertex_passes == 2
    assert psdr.launch_plan_mt((257, 257, 2)).cell_passes == 1 and psdr.launch_plan_mt((257, 258, 2)).cell_passes == 2


def test_lattice_points_are_the_checkers(psdr):
    import torch
    for shape, lo, hi in (((3, 4, 5), -1.0, 1.0), ((12, 11, 10), -1.0, 1.0), ((2, 3, 2), (0.0, -1.0, 2.0), (1.0, 1.5, 2.5))):
        p = psdr.lattice_points(shape, lo, hi)
        assert p.dtype == torch.float32 and not p.is_cuda and np.array_equal(p.numpy(), ref.lattice(shape, lo, hi))
    p = psdr.lattice_points((3, 2, 2), 0.0, 1.0).numpy()
    assert p[1].tolist() == [0.5, 0.0, 0.0] and p[3].tolist() == [0.0, 1.0, 0.0] and p[6].tolist() == [0.0, 0.0, 1.0]          # u = x + nx (y + ny z)
    for bad in (((3, 2, 2), 1.0, 1.0), ((3, 2, 2), 0.0, float("nan")), ((3, 2, 2), (0, 0), 1.0), ((3, 1, 2), 0.0, 1.0)):
        with pytest.raises(ValueError):
            psdr.lattice_points(*bad)


def test_every_entry_point_refuses_bad_arguments_before_any_device_call(psdr):
    """no GPU is visible here: a call that reached the device would fail with a HIP error, not with the entry point's own message.  The non-NULL device pointers are host
    addresses that a refused call never reads."""
    from psdr_jit_amd import cabi
    L = cabi.lib()
    host = np.zeros(512, dtype=np.int64)
    p = [host.ctypes.data + 64 * i for i in range(30)]
    one_more = (97, 257, 673)
    assert one_more[0] * one_more[1] * one_more[2] == 2 ** 24 + 1       # Nv = 2^24 + 1 with every extent above 1
    shapes_refused = (((1, 4, 4), "at least 2"), ((4, 1, 4), "at least 2"), ((4, 4, 1), "at least 2"), ((4, 4, 0), "at least 2"), ((-3, 4, 4), "at least 2"),
                      (one_more, "2^24"), ((4097, 4096, 2), "2^24"), ((2 ** 23 + 1, 2, 2), "2^24"), ((2 ** 30, 2 ** 30, 2 ** 30), "2^24"))

    def refused(rc, name, word):
        msg = L.psdr_hip_last_error().decode()
        assert rc != 0 and msg.startswith(name + ":") and word in msg and "hip" not in msg[len(name):].lower(), (name, word, rc, msg)

    def check(name, keys, call):
        for shape, word in shapes_refused:
            refused(call(shape=shape), name, word)
        for key in keys:
            refused(call(**{key: None}), name, "NULL")

    name = "psdr_hip_mtet_plan"
    outs = [C.c_int32() for _ in range(6)]
    for shape, word in shapes_refused:
        refused(L.psdr_hip_mtet_plan(*shape, *[C.byref(o) for o in outs]), name, word)
    for k in range(6):
        refused(L.psdr_hip_mtet_plan(4, 4, 4, *[None if i == k else C.byref(o) for i, o in enumerate(outs)]), name, "NULL")
    # exactly 2^24 lattice vertices is accepted, one more row is not
    assert L.psdr_hip_mtet_plan(256, 256, 256, *[C.byref(o) for o in outs]) == 0
    refused(L.psdr_hip_mtet_plan(256, 256, 257, *[C.byref(o) for o in outs]), name, "2^24")

    name = "psdr_hip_mtet_count"
    keys = ("sdf", "mask", "base", "cell_faces", "cell_base", "scratch", "totals")

    def count(shape=(4, 4, 4), **change):
        a = {k: p[i] for i, k in enumerate(keys)}
        a.update(change)
        return L.psdr_hip_mtet_count(a["sdf"], *shape, *[a[k] for k in keys[1:]], None)

    check(name, keys, count)
    refused(count(base=p[1]), name, "of their own")
    refused(count(totals=p[5]), name, "of their own")
    refused(count(mask=p[0]), name, "of their own")

    name = "psdr_hip_mtet_emit"
    keys = ("sdf", "mask", "base", "cell_base", "edges", "faces")

    def emit(shape=(4, 4, 4), V=5, F=4, edge_rows=None, face_rows=None, **change):
        a = {k: p[i] for i, k in enumerate(keys)}
        a.update(change)
        return L.psdr_hip_mtet_emit(a["sdf"], *shape, a["mask"], a["base"], a["cell_base"], V, F, a["edges"], V if edge_rows is None else edge_rows,
                                    a["faces"], F if face_rows is None else face_rows, None)

    check(name, keys, emit)
    refused(emit(V=0), name, "num_vertices = 0")
    refused(emit(V=7 * 64 + 1), name, "num_vertices = ")
    refused(emit(F=0), name, "num_faces = 0")
    refused(emit(F=12 * 27 + 1), name, "num_faces = ")
    refused(emit(edge_rows=4), name, "disagrees")                       # totals that disagree with the sizes given
    refused(emit(face_rows=5), name, "disagrees")
    refused(emit(faces=p[4]), name, "of their own")
    refused(emit(edges=p[2]), name, "of their own")

    name = "psdr_hip_mtet_vertices"
    keys = ("sdf", "pos", "edges", "v")

    def vertices(shape=(4, 4, 4), V=5, **change):
        a = {k: p[i] for i, k in enumerate(keys)}
        a.update(change)
        return L.psdr_hip_mtet_vertices(a["sdf"], a["pos"], *shape, a["edges"], V, a["v"], None)

    check(name, keys, vertices)
    refused(vertices(V=0), name, "num_vertices = 0")
    refused(vertices(V=-1), name, "num_vertices = -1")
    refused(vertices(v=p[1]), name, "of its own")

    name = "psdr_hip_mtet_vertices_adj"
    keys = ("sdf", "pos", "mask", "base", "g", "gs", "gp")

    def adj(shape=(4, 4, 4), V=5, **change):
        a = {k: p[i] for i, k in enumerate(keys)}
        a.update(change)
        return L.psdr_hip_mtet_vertices_adj(a["sdf"], a["pos"], *shape, a["mask"], a["base"], V, a["g"], a["gs"], a["gp"], None)

    check(name, keys, adj)
    refused(adj(V=0), name, "num_vertices = 0")
    refused(adj(gs=p[6]), name, "of their own")
    refused(adj(gp=p[0]), name, "of their own")
    refused(adj(gs=p[4]), name, "of their own")
    assert not host.any()


def test_python_surface_refusals(psdr):
    """wrong arguments are a ValueError before a device is looked for (there is none here); mt(...) before any extract raises"""
    import torch
    for shape in ((1, 4, 4), (4, 4, 1), (4, 4), (4, 4, 4, 4), (4.0, 4, 4), ("4", 4, 4), None, 4, (True, 4, 4), (97, 257, 673), (257, 65281, 2), (2 ** 24 + 1, 1, 1)):
        with pytest.raises(ValueError):
            psdr.MarchingTetrahedra(shape)
        with pytest.raises(ValueError):
            psdr.launch_plan_mt(shape)
    with pytest.raises(ValueError):
        psdr.MarchingTetrahedra((4097, 4096, 2))                         # Nv > 2^24
    assert psdr.MarchingTetrahedra((256, 256, 256)).num_lattice == 2 ** 24
    mt = psdr.MarchingTetrahedra((3, 4, 5))
    assert mt.shape == (3, 4, 5) and mt.num_lattice == 60 and mt.topology is None
    good_s, good_p = torch.zeros(60), torch.zeros(60, 3)
    bad_sdf = (torch.zeros(60, dtype=torch.int32), torch.zeros(60, dtype=torch.int64), torch.zeros(59), torch.zeros(60, 1), torch.zeros(5, 4, 3), np.zeros(60, np.int64))
    bad_pos = (torch.zeros(60, 2), torch.zeros(59, 3), torch.zeros(60, 3, dtype=torch.int32), torch.zeros(180), torch.zeros(3, 60))
    for bad in bad_sdf:
        with pytest.raises(ValueError):
            mt.extract(bad)
        with pytest.raises(ValueError):
            mt(bad, good_p)
        with pytest.raises(ValueError):
            mt.vjp(bad, good_p, torch.zeros(0, 3))
    for bad in bad_pos:
        with pytest.raises(ValueError):
            mt(good_s, bad)
        with pytest.raises(ValueError):
            mt.vjp(good_s, bad, torch.zeros(0, 3))
    # before any extract: an error of its own, not a missing device
    for call in (lambda: mt(good_s, good_p), lambda: mt.vjp(good_s, good_p, torch.zeros(0, 3)), lambda: mt.to_mesh(torch.zeros(0, 3))):
        with pytest.raises(RuntimeError, match="extract"):
            call()
