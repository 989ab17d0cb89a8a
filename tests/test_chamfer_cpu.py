"""The Chamfer distance and the surface sampler, what can be checked without a GPU: the Python launch_plan equals psdr_hip_chamfer_plan over a sweep of sizes and on the
plan's own boundaries, and its slices tile [0, m) exactly once; the entry points are declared, exported and listed and refuse bad arguments before they touch a device;
the Python surface refuses wrong arguments before it looks for one; SurfaceSampler's draw on the host (weights, seed, the stratified counts, zero-area faces, the exact
transpose); and the checker itself against finite differences."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import chamfer_ref as ref
import subdiv_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("psdr_hip_chamfer_plan", "psdr_hip_chamfer_nearest", "psdr_hip_chamfer_eval")
SWEEP = (1, 63, 64, 65, 255, 256, 257, 1000, 4097, 40962, 163842, 1 << 26)


@pytest.fixture(scope="module")
def psdr():
    import __graft_entry__
    __graft_entry__.build()
    import psdr_jit_amd
    return psdr_jit_amd


def _c_plan(L, n, m):
    out = [C.c_int32() for _ in range(4)]
    assert L.psdr_hip_chamfer_plan(n, m, *[C.byref(o) for o in out]) == 0, L.psdr_hip_last_error().decode()
    return tuple(o.value for o in out)


def test_plan_python_equals_c_and_slices_tile_the_candidates(psdr):
    from psdr_jit_amd import cabi
    L, plan = cabi.lib(), psdr.launch_plan
    top = 1 << 26
    ns = set(SWEEP) | set(ref.query_sizes(plan))
    ms = set(SWEEP) | set(ref.candidate_sizes(plan))
    # the plan's own boundaries +- 1: where queries_per_lane switches, and for several n where a slice first holds more than one tile and a multiple of slice_len there
    nm = ref.narrow_max(plan)
    ns |= {n for n in (nm - 1, nm, nm + 1) if 1 <= n <= top}
    for n in (1, 65, nm, nm + 1, 40962):
        if n > top or plan(n, top).slice_len == plan(n, 1).tile:
            continue
        edge = ref.first_long_slice(plan, n)
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
            # the slices [s length, min(m, (s + 1) length)) cover [0, m) exactly once and none is empty
            assert (slices - 1) * length < m <= slices * length, (n, m, p)
            assert 256 * q * -(-n // (256 * q)) >= n
            seen_q.add(q)
            seen_long |= length > tile
    assert len(seen_q) >= 2 and seen_long          # (the sweep reaches both scans and slices of more than one tile)
    for n, m in ((0, 1), (1, 0), (-1, 5), (top + 1, 1), (1, top + 1)):
        with pytest.raises(ValueError):
            plan(n, m)


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
    for name in ("ChamferDistance", "SurfaceSampler", "nearest_points", "launch_plan"):
        assert hasattr(psdr, name)
    units = {u[0]: u for u in build.hip_units()}
    assert units["chamfer"][1].endswith("chamfer.hip") and units["chamfer"][1] in build.HIP_SRCS
    names = [u[0] for u in build.hip_units()]
    assert names.index("meshreg") + 1 == names.index("chamfer") and names.index("ssim") + 1 == names.index("meshreg")
    deps = {os.path.relpath(d, ROOT) for d in units["chamfer"][3]}
    assert {os.path.join("include", "psdr_hip.h"), os.path.join("psdr_jit_amd", "csrc", "hip", "nn_scan.h"), os.path.join("psdr_jit_amd", "csrc", "hip", "op_common.h"), os.path.join("psdr_jit_amd", "isa_lint.py")} <= deps
    contract = text[text.index("THE STREAM CONTRACT"):text.index("const char *psdr_hip_last_error")]
    assert "psdr_hip_chamfer_nearest" in contract and "psdr_hip_chamfer_eval" in contract and "psdr_hip_chamfer_plan" in contract


def test_every_entry_point_refuses_bad_arguments_before_any_device_call(psdr):
    """no GPU is visible here: a call that reached the device would fail with a HIP error, not with the entry point's own message.  The non-NULL device pointers are host
    addresses that a refused call never reads."""
    from psdr_jit_amd import cabi
    L = cabi.lib()
    host = np.zeros(256, dtype=np.int64)
    p = [host.ctypes.data + 64 * i for i in range(20)]
    top = 1 << 26

    def refused(rc, name, word):
        msg = L.psdr_hip_last_error().decode()
        assert rc != 0 and msg.startswith(name + ":") and word in msg and "hip" not in msg[len(name):].lower(), (name, word, rc, msg)

    name = "psdr_hip_chamfer_plan"
    o = [C.c_int32() for _ in range(4)]
    for n, m, word in ((0, 1, "n = 0"), (1, 0, "m = 0"), (top + 1, 1, "n = "), (1, -3, "m = -3")):
        refused(L.psdr_hip_chamfer_plan(n, m, *[C.byref(v) for v in o]), name, word)
    refused(L.psdr_hip_chamfer_plan(1, 1, None, C.byref(o[1]), C.byref(o[2]), C.byref(o[3])), name, "NULL")
    name = "psdr_hip_chamfer_nearest"
    fn = L.psdr_hip_chamfer_nearest
    for n, m, word in ((0, 1, "n = 0"), (1, 0, "m = 0"), (top + 1, 1, "n = "), (1, top + 1, "m = ")):
        refused(fn(p[0], n, p[1], m, p[2], p[3], p[4], None), name, word)
    for k in range(5):
        args = [p[0], p[1], p[2], p[3], p[4]]
        args[k] = None
        refused(fn(args[0], 4, args[1], 4, args[2], args[3], args[4], None), name, "NULL")
    name = "psdr_hip_chamfer_eval"
    fn = L.psdr_hip_chamfer_eval
    w = lambda *a: (C.c_float * 2)(*a)

    def call(n=4, m=4, weights=w(1, 1), **change):
        a = dict(x=p[0], y=p[1], ixy=p[2], dxy=p[3], iyx=p[4], dyx=p[5], xb=p[6], xl=p[7], yb=p[8], yl=p[9], partial=p[10], out=p[11], gx=p[12], gy=p[13])
        a.update(change)
        return fn(a["x"], n, a["y"], m, a["ixy"], a["dxy"], a["iyx"], a["dyx"], a["xb"], a["xl"], a["yb"], a["yl"], weights, 1, a["partial"], a["out"], a["gx"], a["gy"], None)

    refused(call(n=0), name, "n = 0")
    refused(call(m=top + 1), name, "m = ")
    for key in ("x", "y", "partial", "out"):
        refused(call(**{key: None}), name, "NULL")
    refused(call(weights=None), name, "NULL")
    for k, bad in ((0, -1.0), (1, float("nan")), (1, float("inf"))):
        ws = [1.0, 1.0]
        ws[k] = bad
        refused(call(weights=w(*ws)), name, "weights[%d]" % k)
    refused(call(gx=None), name, "both")
    refused(call(gy=None), name, "both")
    refused(call(gx=p[0]), name, "of their own")
    refused(call(gy=p[12]), name, "of their own")
    refused(call(ixy=None), name, "index_xy")
    refused(call(dyx=None), name, "index_yx")
    refused(call(yb=None), name, "y_begin")
    refused(call(xl=None), name, "x_begin")
    assert not host.any()


def test_python_surface_refusals(psdr):
    """wrong arguments are a ValueError before a device is looked for (there is none here)"""
    import torch
    good = torch.zeros(5, 3)
    for weights in ((1.0,), (1.0, -1.0), (1.0, float("nan")), (float("inf"), 0.0), 1.0, ("a", 1), (1.0, 1.0, 1.0)):
        with pytest.raises(ValueError):
            psdr.ChamferDistance(weights=weights)
    cd = psdr.ChamferDistance()
    assert cd.weights == (1.0, 1.0) and cd.squared is True
    bad_points = (torch.zeros(5, 2), torch.zeros(0, 3), torch.zeros(5, 3, dtype=torch.int32), torch.zeros(5), torch.zeros(2, 5, 3), np.zeros((4, 3), np.int64))
    for bad in bad_points:
        for args in ((bad, good), (good, bad)):
            with pytest.raises(ValueError):
                cd(*args)
            with pytest.raises(ValueError):
                cd.value_and_grad(*args)
            with pytest.raises(ValueError):
                psdr.nearest_points(*args)
    cd.weights = (1.0, -2.0)                                  # the attributes are read at every call
    with pytest.raises(ValueError):
        cd(good, good)
    f = np.array(sref.grid(3)[0])
    for args, kw in (((f,), {}), ((f, 0), {}), ((f, 8), {}), ((f[:, :2], 9), {}), ((f.astype(np.float64), 9), {}), ((np.array([[0, 1, 1]]), 3), {}),
                     ((np.zeros((0, 3), np.int64), 3), {}), ((f, 9), dict(num_points=0)), ((f, 9), dict(num_points=2.5)), ((f, 9), dict(num_points=(1 << 26) + 1))):
        with pytest.raises(ValueError):
            psdr.SurfaceSampler(*args, **kw)
    sam = psdr.SurfaceSampler(f, 9, num_points=10)
    with pytest.raises(ValueError):
        sam(torch.zeros(9, 3))                                 # before the first resample
    with pytest.raises(ValueError):
        sam.resample(np.zeros((8, 3)))
    with pytest.raises(ValueError):
        sam.resample(np.full((9, 3), np.nan))
    sam.resample(ref._uniform(9, 1))
    for bad in (torch.zeros(9, 2), torch.zeros(8, 3), torch.zeros(9, 3, dtype=torch.int64)):
        with pytest.raises(ValueError):
            sam(bad)


def _areas(v, f):
    v = np.asarray(v, np.float64)
    return 0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)


def _check_draw(sam, v, f, n):
    P = sam.num_points
    rb, col, w = sam.csr()
    assert sam.faces.shape == (P,) and sam.faces.dtype == np.int32 and sam.bary.shape == (P, 3)
    assert rb.dtype == col.dtype == np.int32 and w.dtype == np.float32 and np.array_equal(rb, 3 * np.arange(P + 1)) and col.shape == w.shape == (3 * P,)
    # three non-negative weights summing to 1 within 2 ulp, on the drawn face's vertices
    assert (w >= 0).all() and np.abs(w.reshape(P, 3).astype(np.float64).sum(1) - 1.0).max() <= 2 * 2.0 ** -23
    assert np.array_equal(col.reshape(P, 3), f[sam.faces])
    assert np.array_equal(w.reshape(P, 3), sam.bary.astype(np.float32))
    # the stratified inversion: |count_f - P area_f / total| < 2, and nothing on a face of zero area; faces ascend
    area = _areas(v, f)
    count = np.bincount(sam.faces, minlength=len(f))
    assert np.abs(count - P * area / area.sum()).max() < 2
    assert not count[area == 0].any()
    assert (np.diff(sam.faces) >= 0).all()
    # the transpose CSR is the exact transpose: the same (row, column, value) triples, rows ascending inside a column
    trb, tcol, tw = sam.csr(transpose=True)
    assert trb.shape == (n + 1,) and trb[0] == 0 and trb[-1] == 3 * P and tw.dtype == np.float32
    rows = np.repeat(np.arange(P), 3)
    t_rows = np.repeat(np.arange(n), np.diff(trb))
    assert sorted(zip(rows.tolist(), col.tolist(), w.tolist())) == sorted(zip(tcol.tolist(), t_rows.tolist(), tw.tolist()))
    assert all((np.diff(tcol[trb[i]:trb[i + 1]]) >= 0).all() for i in range(n))


def test_surface_sampler_on_the_host(psdr):
    # areas spanning 1 : 1000: a strip of triangles whose widths grow geometrically
    k = 12
    width = np.concatenate([[0.0], np.cumsum(1000.0 ** (np.arange(k) / (k - 1.0)))])
    v = np.concatenate([np.stack([width, np.zeros(k + 1), np.zeros(k + 1)], 1), np.stack([width, np.ones(k + 1), 0.1 * np.arange(k + 1)], 1)])
    f = np.array([[i, i + 1, k + 1 + i] for i in range(k)] + [[i + 1, k + 2 + i, k + 1 + i] for i in range(k)])
    area = _areas(v, f)
    assert area.max() / area.min() >= 1000
    sam = psdr.SurfaceSampler(f, len(v), num_points=5000, seed=3).resample(v)
    _check_draw(sam, v, f, len(v))
    # the same seed gives the same draw; another seed another; a second resample draws anew
    again = psdr.SurfaceSampler(f, len(v), num_points=5000, seed=3).resample(v)
    assert np.array_equal(again.faces, sam.faces) and np.array_equal(again.bary, sam.bary) and all(np.array_equal(a, b) for a, b in zip(again.csr(), sam.csr()))
    other = psdr.SurfaceSampler(f, len(v), num_points=5000, seed=4).resample(v)
    assert not np.array_equal(other.bary, sam.bary)
    first = sam.bary.copy()
    sam.resample(v)
    assert not np.array_equal(first, sam.bary)
    _check_draw(sam, v, f, len(v))
    # the points are on the surface and uniform on it: their mean is the area-weighted mean of the face centroids within 5 standard errors of a UNIFORM draw (the
    # stratified draw has less variance)
    rb, col, w = sam.csr()
    pts = (w.reshape(-1, 3, 1).astype(np.float64) * v[col.reshape(-1, 3)]).sum(1)
    cen = v[f].mean(1)
    want = (area[:, None] * cen).sum(0) / area.sum()
    spread = np.sqrt(((area[:, None] * (cen - want) ** 2).sum(0) / area.sum()) + (v.max(0) - v.min(0)) ** 2 / 18.0)
    assert (np.abs(pts.mean(0) - want) <= 5 * spread / np.sqrt(sam.num_points) + 1e-12).all()
    # a mesh with a zero-area face (vertex 4 sits on the edge 1 - 2) and an unused vertex: it draws nothing
    v2 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.3, 0.2, 1.0], [0.5, 0.5, 0.0], [9, 9, 9]], np.float64)
    f2 = np.array([[0, 1, 2], [1, 4, 2], [0, 3, 1], [2, 3, 0]])
    assert _areas(v2, f2)[1] == 0
    sam2 = psdr.SurfaceSampler(f2, 6, num_points=777, seed=0).resample(v2)
    _check_draw(sam2, v2, f2, 6)
    assert not (sam2.faces == 1).any()
    # a Mesh-like object works as well; float32 tensors are snapshots
    import torch
    mesh = type("M", (), {"face_indices": f2.astype(np.int32), "num_vertices": 6})()
    sam3 = psdr.SurfaceSampler(mesh, num_points=777, seed=0).resample(torch.from_numpy(v2))
    assert np.array_equal(sam3.faces, sam2.faces) and np.array_equal(sam3.bary, sam2.bary)
    # a mesh of zero total area raises
    flat = v2.copy()
    flat[:, 1:] = 0
    with pytest.raises(ValueError):
        psdr.SurfaceSampler(f2, 6, num_points=10).resample(flat)


@pytest.mark.parametrize("squared", [True, False])
def test_checker_against_finite_differences(squared):
    """the float64 evaluate on a jittered lattice of spacing 0.25, y near a part of x's points: the margins between a nearest and a second nearest neighbour are of the
    jitter's order, 1e-2, far above h = 1e-6, so that no index flips - which is asserted at every displaced point"""
    r = np.random.default_rng(5)
    g = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(3), indexing="ij"), -1).reshape(-1, 3) * 0.25
    x = g + r.uniform(-0.02, 0.02, g.shape)
    y = np.concatenate([g[:40] + r.uniform(-0.02, 0.02, (40, 3)), g[5:25] + r.uniform(-0.02, 0.02, (20, 3))])          # 20 of x's points are chosen twice, 8 never
    w = (1.0, 0.5)

    def indices(x, y):
        d = ((x[:, None, :] - y[None, :, :]) ** 2).sum(2)
        return d.argmin(1), d.argmin(0)

    a, b = indices(x, y)
    assert len(set(b.tolist())) < len(y)
    res = ref.evaluate(x, y, a, b, w, squared)
    assert res["loss"] > 0 and res["terms"][0] > 0 and res["terms"][1] > 0
    assert res["loss"] == pytest.approx(w[0] * res["terms"][0] + w[1] * res["terms"][1], rel=1e-15)
    h = 1e-6
    for which, grad in ((0, res["gx"]), (1, res["gy"])):
        fd = np.zeros_like(grad)
        for i in range(grad.shape[0]):
            for c in range(3):
                vals = []
                for s in (+1, -1):
                    p = [x.copy(), y.copy()]
                    p[which][i, c] += s * h
                    a2, b2 = indices(*p)
                    assert np.array_equal(a2, a) and np.array_equal(b2, b)          # no index flipped
                    vals.append(ref.evaluate(p[0], p[1], a2, b2, w, squared)["loss"])
                fd[i, c] = (vals[0] - vals[1]) / (2 * h)
        assert np.abs(fd - grad).max() <= 1e-8 * max(np.abs(grad).max(), 1.0), (which, np.abs(fd - grad).max())
    # one direction alone, and the float32 reading of the same statements
    only = ref.evaluate(x, y, a, None, (1.0, 0.0), squared)
    assert only["terms"][1] == 0 and only["loss"] == only["terms"][0] == res["terms"][0]
    f32 = ref.evaluate(x.astype(np.float32), y.astype(np.float32), a, b, w, squared, np.float32)
    assert f32["gx"].dtype == np.float32 and np.abs(f32["gx"] - res["gx"]).max() <= 1e-5 * np.abs(res["gx"]).max()
    # rho' at 0 is 0: a point that sits on its nearest neighbour adds no gradient in either mode
    z = ref.evaluate(x, x.copy(), np.arange(len(x)), np.arange(len(x)), w, squared)
    assert z["loss"] == 0 and not z["gx"].any() and not z["gy"].any()


def test_float32_nearest_is_the_definition(psdr):
    """the chunked scan equals a per-pair loop in the definition's operation order on a case with exact ties; the lowest index wins; the far case tells the expansion form
    from the difference form"""
    r = np.random.default_rng(2)
    x, y = (r.integers(0, 4, (40, 3)) / 64.0).astype(np.float32), (r.integers(0, 4, (90, 3)) / 64.0).astype(np.float32)
    idx, d2 = ref.nearest(x, y)
    for i in range(len(x)):
        best, at = np.float32(np.inf), -1
        for j in range(len(y)):
            dx, dy, dz = x[i, 0] - y[j, 0], x[i, 1] - y[j, 1], x[i, 2] - y[j, 2]
            d = (dx * dx + dy * dy) + dz * dz
            assert d.dtype == np.float32
            if d < best:
                best, at = d, j
        assert (idx[i], d2[i]) == (at, best)
    fx, fy, fa, _fd, _fb, _ = ref.reference("far", psdr.launch_plan)
    assert (ref.nearest_expansion(fx, fy) != fa).any()
