"""The point-to-mesh distance, what can be checked without a GPU: the entry points are declared, exported and listed and the unit is a row of the build; the Python
launch_plan_pm equals psdr_hip_pointmesh_plan over a sweep of sizes and on the plan's own boundaries, and its slices tile the candidates exactly once; the entry points and
the Python surface refuse wrong arguments before they touch a device; and the checker itself (tests/pointmesh_ref.py): the cascade against a second, independent
formulation on every named case, the census of the seven regions, the degenerate case in float32, and the gradients against finite differences."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import chamfer_ref as cref
import pointmesh_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("psdr_hip_pointmesh_plan", "psdr_hip_pointmesh_nearest", "psdr_hip_pointmesh_eval")
SWEEP = (1, 63, 64, 65, 255, 256, 257, 1000, 4097, 40962, 163842, 1 << 26)


@pytest.fixture(scope="module")
def psdr():
    import __graft_entry__
    __graft_entry__.build()
    import psdr_jit_amd
    return psdr_jit_amd


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
    assert "THE POINT-TO-MESH DISTANCE" in text
    assert re.search(r"#define\s+PSDR_HIP_ABI_VERSION\s+16\b", text) and L.psdr_hip_abi_version() == 16          # additive: the ABI stays at 16
    for name in ("PointMeshDistance", "closest_points_on_mesh", "launch_plan_pm"):
        assert hasattr(psdr, name)
    units = {u[0]: u for u in build.hip_units()}
    assert units["pointmesh"][1].endswith("pointmesh.hip") and units["pointmesh"][1] in build.HIP_SRCS
    assert [u[0] for u in build.OPERATOR_UNITS][-1] == "pointmesh" and [u[0] for u in build.hip_units()].count("pointmesh") == 1 and [u[0] for u in build.hip_units()][-1] == "pointmesh"
    deps = {os.path.relpath(d, ROOT) for d in units["pointmesh"][3]}
    assert {os.path.join("include", "psdr_hip.h"), os.path.join("psdr_jit_amd", "csrc", "hip", "mesh_pair.h"), os.path.join("psdr_jit_amd", "csrc", "hip", "nn_scan.h"), os.path.join("psdr_jit_amd", "csrc", "hip", "op_common.h"), os.path.join("psdr_jit_amd", "isa_lint.py")} <= deps
    contract = text[text.index("THE STREAM CONTRACT"):text.index("const char *psdr_hip_last_error")]
    assert all(name in contract for name in NEW)


def _c_plan(L, n, m):
    out = [C.c_int32() for _ in range(4)]
    assert L.psdr_hip_pointmesh_plan(n, m, *[C.byref(o) for o in out]) == 0, L.psdr_hip_last_error().decode()
    return tuple(o.value for o in out)


def test_plan_python_equals_c_and_slices_tile_the_candidates(psdr):
    """the boundary finders of tests/chamfer_ref.py read any plan of this shape: nothing here is a copy of the plan's constants"""
    from psdr_jit_amd import cabi
    L, plan = cabi.lib(), psdr.launch_plan_pm
    top = 1 << 26
    ns = set(SWEEP) | set(cref.query_sizes(plan))
    ms = set(SWEEP) | set(cref.candidate_sizes(plan))
    nm = cref.narrow_max(plan)
    ns |= {n for n in (nm - 1, nm, nm + 1) if 1 <= n <= top}
    for n in (1, 65, nm, nm + 1, 40962):
        if n > top or plan(n, top).slice_len == plan(n, 1).tile:
            continue
        edge = cref.first_long_slice(plan, n)
        length = plan(n, edge).slice_len
        ms |= {m for m in (edge - 1, edge, edge + 1, 3 * length - 1, 3 * length, 3 * length + 1) if 1 <= m <= top}
    assert len(ns) >= 15 and len(ms) >= 15
    seen_q, seen_long = set(), False
    for n in sorted(ns):
        for m in sorted(ms):
            p = plan(n, m)
            assert tuple(p) == _c_plan(L, n, m), (n, m)
            tile, q, slices, length = p
            assert tile >= 1 and q >= 1 and slices >= 1 and length % tile == 0 and length >= tile
            assert (slices - 1) * length < m <= slices * length, (n, m, p)          # the slices cover [0, m) exactly once and none is empty
            assert 256 * q * -(-n // (256 * q)) >= n
            seen_q.add(q)
            seen_long |= length > tile
    assert len(seen_q) >= 2 and seen_long
    for n, m in ((0, 1), (1, 0), (-1, 5), (top + 1, 1), (1, top + 1)):
        with pytest.raises(ValueError):
            plan(n, m)


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

    name = "psdr_hip_pointmesh_plan"
    o = [C.c_int32() for _ in range(4)]
    for n, m, word in ((0, 1, "n_queries = 0"), (1, 0, "n_candidates = 0"), (top + 1, 1, "n_queries = "), (1, -3, "n_candidates = -3")):
        refused(L.psdr_hip_pointmesh_plan(n, m, *[C.byref(v) for v in o]), name, word)
    refused(L.psdr_hip_pointmesh_plan(1, 1, None, C.byref(o[1]), C.byref(o[2]), C.byref(o[3])), name, "NULL")

    name = "psdr_hip_pointmesh_nearest"
    fn = L.psdr_hip_pointmesh_nearest

    def near(N=4, n=4, F=4, direction=0, **change):
        a = dict(p=p[0], v=p[1], faces=p[2], records=p[3], keys=p[4], index=p[5], bary=p[6], dist2=p[7])
        a.update(change)
        return fn(a["p"], N, a["v"], n, a["faces"], F, direction, a["records"], a["keys"], a["index"], a["bary"], a["dist2"], None)

    refused(near(N=0), name, "n_points = 0")
    refused(near(n=top + 1), name, "n_vertices = ")
    refused(near(F=-2), name, "n_faces = -2")
    refused(near(direction=2), name, "direction = 2")
    for key in ("p", "v", "faces", "keys", "index", "bary", "dist2"):
        for direction in (0, 1):
            refused(near(direction=direction, **{key: None}), name, "NULL")
    refused(near(records=None), name, "records")

    name = "psdr_hip_pointmesh_eval"
    fn = L.psdr_hip_pointmesh_eval
    w = lambda *a: (C.c_float * 2)(*a)
    keys = ("p", "v", "faces", "fop", "bp", "dp", "pof", "bf", "df", "pb", "pl", "fb", "fl", "vb", "vc", "partial", "corners", "out", "gp", "gv")

    def call(N=4, n=4, F=4, weights=w(1, 1), **change):
        a = {k: p[i] for i, k in enumerate(keys)}
        a.update(change)
        return fn(a["p"], N, a["v"], n, a["faces"], F, a["fop"], a["bp"], a["dp"], a["pof"], a["bf"], a["df"], a["pb"], a["pl"], a["fb"], a["fl"], a["vb"], a["vc"],
                  weights, 1, a["partial"], a["corners"], a["out"], a["gp"], a["gv"], None)

    refused(call(N=0), name, "n_points = 0")
    refused(call(n=0), name, "n_vertices = 0")
    refused(call(F=top + 1), name, "n_faces = ")
    for key in ("p", "v", "faces", "partial", "out"):
        refused(call(**{key: None}), name, "NULL")
    refused(call(weights=None), name, "NULL")
    for k, bad in ((0, -1.0), (1, float("nan")), (1, float("inf"))):
        ws = [1.0, 1.0]
        ws[k] = bad
        refused(call(weights=w(*ws)), name, "weights[%d]" % k)
    refused(call(gp=None), name, "both")
    refused(call(gv=None), name, "both")
    refused(call(gp=p[0]), name, "of their own")
    refused(call(gv=p[18]), name, "of their own")
    for key in ("fop", "bp", "dp"):
        refused(call(**{key: None}), name, "face_of_point")
    for key in ("pof", "bf", "df"):
        refused(call(**{key: None}), name, "point_of_face")
    for key in ("corners", "vb", "vc"):
        refused(call(**{key: None}), name, "vc_begin")
    refused(call(fb=None), name, "f_begin")
    refused(call(pl=None), name, "p_begin")
    assert not host.any()


def test_python_surface_refusals(psdr):
    """wrong arguments are a ValueError before a device is looked for (there is none here)"""
    import torch
    v, f = ref.lattice(8)
    n = len(v)
    for weights in ((1.0,), (1.0, -1.0), (1.0, float("nan")), (float("inf"), 0.0), 1.0, ("a", 1), (1.0, 1.0, 1.0)):
        with pytest.raises(ValueError):
            psdr.PointMeshDistance(f, n, weights=weights)
    for args in ((f,), (f, 0), (f, 3), (f[:, :2], n), (f.astype(np.float64), n), (np.array([[0, 1, 1]]), 3), (np.zeros((0, 3), np.int64), 3)):
        with pytest.raises(ValueError):
            psdr.PointMeshDistance(*args)
    pm = psdr.PointMeshDistance(f, n)
    assert pm.weights == (1.0, 1.0) and pm.squared is True and pm.num_vertices == n and pm.terms is None and pm.nearest is None
    mesh = type("M", (), {"face_indices": f.astype(np.int32), "num_vertices": n})()
    assert np.array_equal(psdr.PointMeshDistance(mesh).faces, f)
    good_p, good_v = torch.zeros(5, 3), torch.from_numpy(v)
    bad_points = (torch.zeros(5, 2), torch.zeros(0, 3), torch.zeros(5, 3, dtype=torch.int32), torch.zeros(5), torch.zeros(2, 5, 3), np.zeros((4, 3), np.int64))
    bad_vertices = (torch.zeros(n - 1, 3), torch.zeros(n, 2), torch.zeros(n, 3, dtype=torch.int64), torch.zeros(n))
    for args in [(bad, good_v) for bad in bad_points] + [(good_p, bad) for bad in bad_vertices]:
        with pytest.raises(ValueError):
            pm(*args)
        with pytest.raises(ValueError):
            pm.value_and_grad(*args)
        with pytest.raises(ValueError):
            psdr.closest_points_on_mesh(args[0], args[1], f)
    for bad in (f[:, :2], f.astype(np.float32), f + n, np.array([[0, 1, 1]]), np.zeros((0, 3), np.int64)):
        with pytest.raises(ValueError):
            psdr.closest_points_on_mesh(good_p, good_v, bad)
    pm.weights = (1.0, -2.0)                                  # the attributes are read at every call
    with pytest.raises(ValueError):
        pm(good_p, good_v)


def _alt_deviation(p, v, f):
    """the worst deviations of closest_alt from the cascade over all pairs, relative to the case's extent: (dist2, q)"""
    A, B, C = ref._corners(v, f)
    size = float(np.abs(np.concatenate([p, v]).astype(np.float64)).max())
    rows = max(1, ref.CHUNK // len(f))
    worst_d = worst_q = 0.0
    for r0 in range(0, len(p), rows):
        _s, _t, d, _r, e = ref.pairs(p[r0:r0 + rows, None, :], A[None], B[None], C[None], np.float64)
        q = p[r0:r0 + rows, None, :].astype(np.float64) - e
        d_alt, q_alt = ref.closest_alt(p[r0:r0 + rows], v, f)
        worst_d = max(worst_d, float((np.abs(d - d_alt) / np.maximum(d, size * size)).max()))
        worst_q = max(worst_q, float(np.abs(q - q_alt).max()) / size)
    return worst_d, worst_q


@pytest.mark.parametrize("name", ref.CASES + ("sweep",))
def test_cascade_agrees_with_the_second_formulation(name):
    """float64: dist2 and the closest point of EVERY pair, to 1e-12 relative"""
    if name == "sweep":
        p, v, f = ref.sweep_reference(2049, 513)[:3]
    else:
        p, v, f = ref.reference(name)[:3]
    worst_d, worst_q = _alt_deviation(p, v, f)
    assert worst_d <= 1e-12 and worst_q <= 1e-12, (name, worst_d, worst_q)


def test_region_census():
    """a condition on the inputs: in the `regions` case every one of the seven regions is the float64 winner's region for at least 32 points"""
    c64 = ref.reference("regions")[3]
    census = np.bincount(c64.region_p, minlength=8)[1:]
    print("regions: the winners' regions 1 .. 7: %s" % census.tolist())
    assert census.shape == (7,) and (census >= 32).all(), census


def test_degenerate_case_is_finite_and_in_range_in_float32():
    p, v, f, c64, c32 = ref.reference("degenerate")
    A, B, C = (x.astype(np.float64) for x in ref._corners(v, f))
    area = 0.5 * np.linalg.norm(np.cross(B - A, C - A), axis=1)
    edges = np.stack([np.linalg.norm(B - A, axis=1), np.linalg.norm(C - B, axis=1), np.linalg.norm(A - C, axis=1)], 1)
    assert (edges.min(1) == 0).sum() == 1 and ((area == 0) & (edges.min(1) > 0)).sum() == 1          # one zero-length edge, one zero-area face with distinct vertices
    assert ((area > 0) & (area < 1e-3 * edges.max(1) ** 2)).sum() == 1                                # one sliver
    for c in (c64, c32):
        assert all(np.isfinite(a).all() for a in (c.dist2_p, c.bary_p, c.dist2_f, c.bary_f))
        assert (c.face_of_point >= 0).all() and (c.face_of_point < len(f)).all() and (c.point_of_face >= 0).all() and (c.point_of_face < len(p)).all()
        assert (c.dist2_p >= 0).all() and (c.dist2_f >= 0).all()
        for b in (c.bary_p, c.bary_f):
            assert b.min() >= -4 * ref.U and b.max() <= 1 + 4 * ref.U and np.abs(b.astype(np.float64).sum(1) - 1).max() <= 4 * ref.U
    # all pairs, float32: nothing but finite numbers, whatever the region
    s, t, d, _r, e = ref.pairs(p[:, None, :], *(x[None] for x in ref._corners(v, f)), np.float32)
    assert np.isfinite(s).all() and np.isfinite(t).all() and np.isfinite(d).all() and np.isfinite(e).all()
    # every degenerate face is somebody's nearest: the case reaches them
    assert {6, 7, 8} <= set(c64.face_of_point.tolist())
    g = ref.evaluate(p, v, f, c32.face_of_point, c32.point_of_face, (1.0, 0.5), False, np.float32)
    assert np.isfinite(g["gp"]).all() and np.isfinite(g["gv"]).all() and np.isfinite(g["loss"])


def test_a_face_whose_a_and_b_coincide():
    """the one arrangement where the cascade does not return the closest point: with ab = 0 test 3 (edge ab) holds for every point that passed tests 1 and 2, and its
    quotient 0 / 0 is 0 by the definition - vertex a: a finite point of the triangle, no NaN, in both precisions"""
    a, c = np.array([0.0, 0.0, 0.0]), np.array([1.0, 0.0, 0.0])
    p = np.array([[0.5, 0.3, 0.0], [2.0, 0.1, 0.0], [-1.0, 0.0, 0.2]])
    for T in (np.float64, np.float32):
        s, t, d, region, _e = ref.pairs(p, a[None], a[None], c[None], T)
        assert np.isfinite(d).all() and not s.any() and not t.any() and region.tolist() == [3, 3, 1]
        assert np.allclose(d, (p * p).sum(1))


@pytest.mark.parametrize("squared", [True, False])
def test_checker_against_finite_differences(squared):
    """evaluate in float64 on the lattice with points well off it, against central differences of the loss ITSELF - the indices are taken anew at every displaced input.
    A point nearest a shared edge is equally near both faces and the index may flip between them under the step; the closest point, hence the loss, is the same through
    either.  The gradient with constant indices AND constant barycentrics equals the derivative: the envelope theorem"""
    v32, f = ref.lattice(18)
    r = np.random.default_rng(7)
    v = v32.astype(np.float64) + r.uniform(-0.01, 0.01, v32.shape)
    p = np.concatenate([r.uniform(-0.1, 1.1, (40, 2)), r.uniform(0.05, 0.4, (40, 1)) * r.choice([-1.0, 1.0], (40, 1))], 1)
    w = (1.0, 0.5)

    def indices(p, v):
        d = ref.matrix(p, v, f)
        return d.argmin(1), d.argmin(0)

    a, b = indices(p, v)
    res = ref.evaluate(p, v, f, a, b, w, squared)
    assert res["loss"] > 0 and res["loss"] == pytest.approx(w[0] * res["terms"][0] + w[1] * res["terms"][1], rel=1e-15)
    h = 1e-6
    for which, grad in ((0, res["gp"]), (1, res["gv"])):
        fd = np.zeros_like(grad)
        for i in range(grad.shape[0]):
            for c in range(3):
                vals = []
                for sgn in (+1, -1):
                    x = [p.copy(), v.copy()]
                    x[which][i, c] += sgn * h
                    a2, b2 = indices(*x)
                    vals.append(ref.evaluate(x[0], x[1], f, a2, b2, w, squared)["loss"])
                fd[i, c] = (vals[0] - vals[1]) / (2 * h)
        assert np.abs(fd - grad).max() <= 2e-8 * max(np.abs(grad).max(), 1.0), (which, np.abs(fd - grad).max())
    only = ref.evaluate(p, v, f, a, None, (1.0, 0.0), squared)
    assert only["terms"][1] == 0 and only["loss"] == only["terms"][0] == res["terms"][0]
    f32 = ref.evaluate(p.astype(np.float32), v.astype(np.float32), f, a, b, w, squared, np.float32)
    assert f32["gv"].dtype == np.float32 and np.abs(f32["gv"] - res["gv"]).max() <= 1e-4 * np.abs(res["gv"]).max()
    # rho' at 0 is 0: points on the mesh's vertices add no gradient in either mode
    z = ref.evaluate(v, v, f, *indices(v, v), w, squared)
    assert z["loss"] == 0 and not z["gp"].any() and not z["gv"].any()
