"""The mesh regularisers, what can be checked without a GPU: psdr.mesh_topology equals the checker's dictionaries (tests/meshreg_ref.py: a per-face loop) on every mesh of
tests/subdiv_ref.py, with the counts the definition implies; the inverted indices are exact transposes; the checker's analytic gradients equal torch float64 autograd of a
short torch statement of the definition to 1e-12 relative, a degenerate face and target_length > 0 included; the three entry points are declared, exported and listed and
refuse bad arguments before they touch a device; the constructor refuses wrong arguments before it looks for one."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import meshreg_ref as ref
import subdiv_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("psdr_hip_meshreg_create", "psdr_hip_meshreg_eval", "psdr_hip_meshreg_destroy")


@pytest.fixture(scope="module")
def psdr():
    import __graft_entry__
    __graft_entry__.build()
    import psdr_jit_amd
    return psdr_jit_amd


def _meshes():
    out = {"tetrahedron": (sref.TETRAHEDRON, 4), "bowtie": (sref.BOWTIE, 5), "book": (sref.BOOK, 5), "fan5": sref.fan(5), "fan70": sref.fan(70), "grid3": sref.grid(3),
           "grid17": sref.grid(17), "twice": ([[0, 1, 2], [2, 0, 1]], 3), "point": ([], 1)}
    f, n, _v = ref.bunny()
    out["bunny"] = (f, n)
    return out


COUNTS = {"book": (7, 0, 6, 1), "grid17": (800, 736, 64, 0), "bunny": (7473, 7431, 42, 0), "tetrahedron": (6, 6, 0, 0), "bowtie": (6, 0, 6, 0), "twice": (3, 3, 0, 0),
          "point": (0, 0, 0, 0), "fan5": (10, 5, 5, 0)}          # edges, hinges, boundary, non-manifold


@pytest.mark.parametrize("name", sorted(_meshes()))
def test_topology_equals_the_checker(psdr, name):
    faces, n = _meshes()[name]
    t = psdr.mesh_topology(np.array(faces, np.int64).reshape(-1, 3), n)
    want = ref.topology(faces, n)
    assert t.edges.dtype == np.int32 and t.hinges.dtype == np.int32 and t.edges.shape == (len(want["edges"]), 2) and t.hinges.shape == (len(want["hinges"]), 4)
    assert [tuple(r) for r in t.edges.tolist()] == want["edges"]
    assert [tuple(r) for r in t.hinges.tolist()] == want["hinges"]
    assert (t.num_boundary_edges, t.num_nonmanifold_edges) == (want["boundary"], want["nonmanifold"])
    if name in COUNTS:
        assert (len(t.edges), len(t.hinges), t.num_boundary_edges, t.num_nonmanifold_edges) == COUNTS[name]
    if name == "twice":
        assert (t.hinges[:, 2] == t.hinges[:, 3]).all()          # two copies of one face: c == d
    # the inverted indices are exact transposes: every (element, role) once, ascending per vertex, under the vertex it names
    for table, begin, elem, role, index in ((t.edges, t.edge_begin, t.edge_elem, t.edge_role, want["edge_index"]),
                                            (t.hinges, t.hinge_begin, t.hinge_elem, t.hinge_role, want["hinge_index"])):
        assert begin.dtype == elem.dtype == role.dtype == np.int32 and begin.shape == (n + 1,) and begin[0] == 0 and begin[-1] == table.size == elem.size == role.size
        got = [list(zip(elem[begin[i]:begin[i + 1]].tolist(), role[begin[i]:begin[i + 1]].tolist())) for i in range(n)]
        assert got == index
        assert all(l == sorted(l) for l in got)
        seen = sorted(p for l in got for p in l)
        assert seen == [(k, r) for k in range(table.shape[0]) for r in range(table.shape[1])]
        assert all(table[k, r] == i for i, l in enumerate(got) for k, r in l)
    # the neighbours are those of the Laplacian pattern the regulariser reuses
    from psdr_jit_amd.precond import laplacian_csr
    rb, col = laplacian_csr(np.array(faces, np.int64).reshape(-1, 3), n)
    assert [col[rb[i]:rb[i + 1]].tolist() for i in range(n)] == want["neighbours"]


def test_topology_refusals(psdr):
    for faces, n in (([[0, 1, 1]], 3), ([[0, 1, 3]], 3), ([[0, -1, 2]], 3), ([[0, 1, 2]], 0), ([[0, 1]], 3), ([[0.0, 1.0, 2.0]], 3)):
        with pytest.raises(ValueError):
            psdr.mesh_topology(np.array(faces), n)


def _torch_statement(V, faces, n, L0):
    """the definition in torch float64 on the CPU, autograd for the gradients; topology from the checker"""
    import torch
    t = ref.topology(faces, n)
    v = torch.from_numpy(np.asarray(V, np.float64)).requires_grad_()
    deg = torch.tensor([len(s) for s in t["neighbours"]], dtype=torch.float64)
    pairs = torch.tensor([(i, j) for i in range(n) for j in t["neighbours"][i]], dtype=torch.int64).reshape(-1, 2)
    mean = torch.zeros(n, 3, dtype=torch.float64).index_add(0, pairs[:, 0], v[pairs[:, 1]]) / deg.clamp(min=1)[:, None]
    lap = (((v - mean) * (deg > 0)[:, None]) ** 2).sum() / max(int((deg > 0).sum()), 1)
    H, E = torch.tensor(t["hinges"], dtype=torch.int64).reshape(-1, 4), torch.tensor(t["edges"], dtype=torch.int64).reshape(-1, 2)
    a, b, c, d = (v[H[:, k]] for k in range(4))
    n1, n2 = torch.linalg.cross(b - a, c - a), torch.linalg.cross(d - a, b - a)
    ok = ((n1 * n1).sum(1) >= ref.TINY) & ((n2 * n2).sum(1) >= ref.TINY)
    u1, u2 = n1[ok] / n1[ok].norm(dim=1, keepdim=True), n2[ok] / n2[ok].norm(dim=1, keepdim=True)
    nor = 0.5 * ((u1 - u2) ** 2).sum() / max(len(H), 1)
    dd = v[E[:, 0]] - v[E[:, 1]]
    l2 = (dd * dd).sum(1)
    live = l2 >= ref.TINY
    edge = (l2.sum() if L0 == 0 else ((l2[live].sqrt() - L0) ** 2).sum() + L0 * L0 * int((~live).sum())) / max(len(E), 1)
    out = {}
    for name, val in (("laplacian", lap), ("normal", nor), ("edge", edge)):
        g, = torch.autograd.grad(val, v, retain_graph=True, allow_unused=True)
        out[name] = (float(val.detach()), np.zeros((n, 3)) if g is None else g.numpy())
    return out


@pytest.mark.parametrize("L0", [0.0, 0.05, 0.7])
@pytest.mark.parametrize("name", ["triangle", "fold", "tetrahedron", "bowtie", "book", "fan5", "fan70", "grid3", "grid17", "degenerate"])
def test_checker_against_torch_autograd(name, L0):
    faces, n, V = ref.case(name)
    got, want = ref.evaluate(V, faces, n, L0), _torch_statement(V, faces, n, L0)
    for term in ref.TERMS:
        assert np.isfinite(got[term][0]) and np.isfinite(got[term][1]).all()
        assert abs(got[term][0] - want[term][0]) <= 1e-12 * max(abs(want[term][0]), 1e-300), (term, got[term][0], want[term][0])
        scale = np.abs(want[term][1]).max()
        assert np.abs(got[term][1] - want[term][1]).max() <= 1e-12 * scale, (term, np.abs(got[term][1] - want[term][1]).max(), scale)
        if name not in ("bowtie", "book", "triangle") or term != "normal":
            assert scale > 0
    if name == "degenerate":
        t = ref.topology(faces, n)
        assert (1, 2, 0, 4) in t["hinges"] and (0, 2, 1, 5) in t["hinges"] and (2, 5) in t["edges"]
        flat = ref.evaluate(V, faces[:2], n, L0)               # the hinges of the two zero-area faces add nothing: only the hinge (0, 1) is left
        assert got["normal"][0] * len(t["hinges"]) == pytest.approx(flat["normal"][0], rel=1e-14)


def test_float32_checker_is_close_and_not_exact():
    """the yardstick exists: e_32 > 0 on the accuracy cases, and e_32 / G stays within float32's reach"""
    for name in ("fold", "fan5", "grid17"):
        f64, f32, _t = ref.reference(name, 0.05)
        for term in ref.TERMS:
            _r, _e, e_32, G = ref.ratio(f64[term][1], f32[term][1], f64[term][1])
            assert f32[term][1].dtype == np.float32 and 0 < e_32 <= 1e-5 * G


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
    assert re.search(r"#define\s+PSDR_HIP_ABI_VERSION\s+16\b", text)
    assert L.psdr_hip_abi_version() == 16
    for name in ("MeshRegularizer", "mesh_topology"):
        assert hasattr(psdr, name)
    units = {u[0]: u for u in build.hip_units()}
    assert units["meshreg"][1].endswith("meshreg.hip") and units["meshreg"][1] in build.HIP_SRCS
    deps = {os.path.relpath(d, ROOT) for d in units["meshreg"][3]}
    assert {os.path.join("include", "psdr_hip.h"), os.path.join("psdr_jit_amd", "csrc", "hip", "op_common.h"), os.path.join("psdr_jit_amd", "isa_lint.py")} <= deps
    # the stream contract names the handle: rule 3 (creates) and rule 5 (handles that own work frames)
    assert re.search(r"\*\s+3\. Every psdr_hip_\*_create \([^)]*meshreg[^)]*\)", text)
    assert re.search(r"\*\s+5\. [^\n]*\n[^\n]*meshreg handle", text)


def test_every_entry_point_refuses_bad_arguments_before_any_device_call(psdr):
    """no GPU is visible here: a call that reached the device would fail with a HIP error, not with the entry point's own message.  The non-NULL device pointers are host
    addresses that a refused call never reads, and so is the handle."""
    from psdr_jit_amd import cabi
    from psdr_jit_amd.precond import laplacian_csr
    L = cabi.lib()
    faces, n = sref.grid(3)
    t = psdr.mesh_topology(np.array(faces), n)
    rb, col = laplacian_csr(np.array(faces), n)
    good = dict(edges=t.edges, hinges=t.hinges, rb=rb, col=col, eb=t.edge_begin, ee=t.edge_elem, er=t.edge_role, hb=t.hinge_begin, he=t.hinge_elem, hr=t.hinge_role)
    order = ("edges", "hinges", "rb", "col", "eb", "ee", "er", "hb", "he", "hr")
    name = "psdr_hip_meshreg_create"
    h = C.c_void_p()

    def refused(rc, name, word):
        msg = L.psdr_hip_last_error().decode()
        assert rc != 0 and msg.startswith(name + ":") and word in msg and "hip" not in msg[len(name):].lower(), (name, word, rc, msg)

    def create(n_=n, e_=len(t.edges), h_=len(t.hinges), out=True, **change):
        arrays = dict(good)
        arrays.update(change)
        keep = [None if arrays[k] is None else np.ascontiguousarray(arrays[k], np.int32) for k in order]
        return L.psdr_hip_meshreg_create(n_, e_, h_, *[None if a is None else a.ctypes.data for a in keep], C.byref(h) if out else None, None)

    def poked(key, index, value):
        a = np.array(good[key], np.int32).copy()
        a.reshape(-1)[index] = value
        return {key: a}

    refused(create(out=False), name, "out is NULL")
    for bad in (0, -1, (1 << 26) + 1):
        refused(create(n_=bad), name, "n = %d" % bad)
    refused(create(e_=-1), name, "e = -1")
    refused(create(h_=-2), name, "h = -2")
    for key, word in (("edges", "edges is NULL"), ("hinges", "hinges is NULL"), ("rb", "row_begin is NULL"), ("col", "col is NULL"), ("eb", "ev_begin is NULL"),
                      ("ee", "ev_elem is NULL"), ("er", "ev_role is NULL"), ("hb", "hv_begin is NULL"), ("he", "hv_elem is NULL"), ("hr", "hv_role is NULL")):
        refused(create(**{key: None}), name, word)
    # an index out of range, in every table
    refused(create(**poked("edges", 1, n)), name, "edge 0")
    refused(create(**poked("edges", 0, -1)), name, "edge 0")
    refused(create(**poked("edges", 2, int(t.edges[1, 1]))), name, "edge 1")          # a == b
    refused(create(**poked("hinges", 2, n)), name, "hinge 0")
    refused(create(**poked("hinges", 7, -1)), name, "hinge 1")
    refused(create(**poked("hinges", 2, int(t.hinges[0, 0]))), name, "hinge 0")       # c on the edge
    refused(create(**poked("col", 3, n)), name, "col[3]")
    refused(create(**poked("col", 0, -1)), name, "col[0]")
    refused(create(**poked("col", 0, 0)), name, "col[0]")                             # the row itself
    refused(create(**poked("ee", 4, len(t.edges))), name, "ev_elem[4]")
    refused(create(**poked("he", 5, -1)), name, "hv_elem[5]")
    # a non-monotone CSR, a CSR that does not start at 0 or end at the right count
    refused(create(**poked("rb", 2, int(rb[3]) + 1)), name, "row_begin is not monotonic")
    refused(create(**poked("rb", 0, 1)), name, "row_begin[0]")
    refused(create(**poked("eb", 3, int(t.edge_begin[4]) + 1)), name, "ev_begin is not monotonic")
    refused(create(**poked("hb", 1, int(t.hinge_begin[2]) + 1)), name, "hv_begin is not monotonic")
    refused(create(**poked("eb", n, 2 * len(t.edges) + 1)), name, "ev_begin ends at")
    refused(create(**poked("hb", n, 4 * len(t.hinges) + 4)), name, "hv_begin ends at")
    # a role out of range, a role or element that names another vertex, entries out of order
    refused(create(**poked("er", 0, 2)), name, "ev_role[0]")
    refused(create(**poked("er", 3, -1)), name, "ev_role[3]")
    refused(create(**poked("hr", 2, 4)), name, "hv_role[2]")
    refused(create(**poked("er", 0, 1 - int(t.edge_role[0]))), name, "which is vertex")
    refused(create(**poked("he", 0, int(t.hinge_elem[0]) + 1)), name, "which is vertex")
    swapped = np.array(t.edge_elem).copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    roles = np.array(t.edge_role).copy()
    roles[[0, 1]] = roles[[1, 0]]
    assert t.edge_begin[1] >= 2
    refused(create(ee=swapped, er=roles), name, "ascending")
    assert not h.value                                        # a refused create leaves no handle behind

    host = np.zeros(64, dtype=np.int64)
    p, p2, p3, p4 = (host.ctypes.data + 64 * i for i in range(4))
    fake = C.c_void_p(p4)                                     # (a refused call never looks into the handle)
    w = lambda *a: (C.c_float * 3)(*a)
    name = "psdr_hip_meshreg_eval"
    fn = L.psdr_hip_meshreg_eval
    refused(fn(None, p, w(1, 1, 1), 0.0, p2, p3, None), name, "handle is NULL")
    refused(fn(fake, None, w(1, 1, 1), 0.0, p2, p3, None), name, "NULL")
    refused(fn(fake, p, None, 0.0, p2, p3, None), name, "NULL")
    refused(fn(fake, p, w(1, 1, 1), 0.0, None, p3, None), name, "NULL")
    refused(fn(fake, p, w(1, 1, 1), 0.0, p2, p, None), name, "grad must be")
    for k, bad in ((0, -1.0), (1, float("nan")), (2, float("inf")), (1, -0.5)):
        ws = [1.0, 1.0, 1.0]
        ws[k] = bad
        refused(fn(fake, p, w(*ws), 0.0, p2, p3, None), name, "weights[%d]" % k)
    for bad in (-0.1, float("nan"), float("inf")):
        refused(fn(fake, p, w(1, 1, 1), bad, p2, p3, None), name, "target_length")
    refused(L.psdr_hip_meshreg_destroy(None), "psdr_hip_meshreg_destroy", "handle is NULL")
    assert not host.any()


def test_constructor_refusals(psdr):
    """wrong arguments are a ValueError before a device is looked for (there is none here)"""
    faces, n = sref.grid(3)
    f = np.array(faces)
    for args, kw in (((f,), {}),                                          # num_vertices missing
                     ((f, 0), {}), ((f, 8), {}), ((f[:, :2], n), {}), ((f.astype(np.float64), n), {}),
                     ((np.array([[0, 1, 1]]), 3), {}), ((np.array([[0, 1, -1]]), 3), {}),
                     ((f, n), dict(weights=(1.0, 1.0))), ((f, n), dict(weights=(1.0, -1.0, 1.0))), ((f, n), dict(weights=(1.0, float("nan"), 1.0))),
                     ((f, n), dict(weights=(float("inf"), 0.0, 0.0))), ((f, n), dict(weights=1.0)), ((f, n), dict(weights=("a", 1, 1))),
                     ((f, n), dict(target_length=-0.1)), ((f, n), dict(target_length=float("nan"))), ((f, n), dict(target_length=float("inf"))),
                     ((f, n), dict(target_length="long"))):
        with pytest.raises(ValueError):
            psdr.MeshRegularizer(*args, **kw)
