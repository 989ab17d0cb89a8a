"""The lattice regularisers, what can be checked without a GPU: the checker itself (tests/latreg_ref.py) - the float64 gradient of each term against central differences, the
edge form of the sign term against the per-vertex form, the exact cases, and the condition that no accuracy case sits on the n = 0 kink of the Eikonal term - then the
plumbing: the entry points are declared, exported and listed, the ABI stays at 16, the unit is the one row of its list between `mtet` and `pointmesh`, the plan of the Python
layer is the library's, and the entry point and the Python surface refuse wrong arguments before they touch a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import latreg_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("psdr_hip_latreg_plan", "psdr_hip_latreg_eval")
UNIT = {"eikonal": (1.0, 0.0, 0.0), "laplacian": (0.0, 1.0, 0.0), "sign": (0.0, 0.0, 1.0)}


@pytest.fixture(scope="module")
def psdr():
    import __graft_entry__
    __graft_entry__.build()
    import psdr_jit_amd
    return psdr_jit_amd


# ---- the checker

def _away_from_zero(sdf, keep):
    return np.where(np.abs(sdf) < keep, np.where(sdf < 0, -keep, keep), sdf)


@pytest.mark.parametrize("term", sorted(UNIT))
@pytest.mark.parametrize("shape", [(4, 3, 5), (2, 3, 2), (3, 3, 3)])
def test_float64_gradient_against_central_differences(term, shape):
    """the step 1e-6 is far below the 0.05 that every value keeps from zero: no displaced input changes a sign, so V stays constant"""
    spacing, k = ref.ACCURACY_SPACING, 3.0
    sdf = _away_from_zero(ref.sphere_noise(shape, spacing, 7).astype(np.float64) + np.random.default_rng(8).normal(0, 0.05, ref.counts(shape)[0]), 0.05)
    base = ref.reference(sdf, shape, spacing, UNIT[term], k)
    if term == "sign":
        assert base["V"] > 0
    h = 1e-6
    fd = np.zeros_like(sdf)
    for u in range(len(sdf)):
        for sgn in (1, -1):
            s = sdf.copy()
            s[u] += sgn * h
            assert np.array_equal(ref.inside(s), ref.inside(sdf))
            fd[u] += sgn * float(ref.reference(s, shape, spacing, UNIT[term], k)["loss"]) / (2 * h)
    g = base["grad"]
    if not (term == "laplacian" and max(shape) < 3):
        assert np.abs(g).max() > 1e-3
    assert np.abs(fd - g).max() <= 1e-6 * max(np.abs(g).max(), 1.0), np.abs(fd - g).max()
    g32 = ref.reference(sdf, shape, spacing, UNIT[term], k, np.float32)["grad"]
    assert g32.dtype == np.float32 and np.abs(g32 - g).max() <= 1e-4 * max(np.abs(g).max(), 1e-3)


@pytest.mark.parametrize("k", ref.SIGN_SCALES)
def test_edge_form_equals_vertex_form(k):
    for shape, seed in (((2, 2, 2), 1), ((2, 3, 5), 2), ((9, 8, 7), 3)):
        for sdf in (ref.pure_noise(shape, seed), ref.sphere_noise(shape, ref.ACCURACY_SPACING, seed)):
            if not ref.crossing_counts(sdf, shape).any():          # (the sphere misses every vertex of the smallest lattices)
                assert min(shape) == 2 and ref.sign_edges(sdf, shape, k) == (0, 0) and ref.sign_vertices(sdf, shape, k)[0] == 0
                continue
            e, Ve = ref.sign_edges(sdf, shape, k)
            v, _g, Vv = ref.sign_vertices(sdf, shape, k)
            assert Ve == Vv and Ve > 0 and abs(e - v) <= 1e-13 * abs(e)
            assert ref.crossing_counts(sdf, shape).max() <= 14
            e32, _ = ref.sign_edges(sdf, shape, k, np.float32)
            v32 = ref.sign_vertices(sdf, shape, k, np.float32)[0]
            assert e32.dtype == np.float32 and v32.dtype == np.float32 and abs(float(e32) - float(v32)) <= 1e-5 * abs(e)


def _exact(shape=(6, 5, 4)):
    X = ref.coords(shape)
    return shape, X, ref.positions(shape, ref.EXACT_SPACING)


def test_exact_cases_on_the_checker():
    shape, X, P = _exact()
    nv, nc = ref.counts(shape)
    h = ref.EXACT_SPACING
    for dtype in (np.float32, np.float64):
        # a linear field: every operation exact
        lin = P[:, 0].astype(np.float32)
        r = ref.reference(lin, shape, h, (1.0, 1.0, 0.0), dtype=dtype)
        assert r["terms"][0] == 0 and r["terms"][1] == 0 and not r["grad"].any()
        # a parabola on integer multiples: r == 2 on the x-interior vertices
        par = (P[:, 0] ** 2).astype(np.float32)
        assert np.array_equal(par.astype(np.float64), P[:, 0] ** 2)
        R = ref.residual(par, shape, h, dtype).ravel()
        interior = (X[:, 0] >= 1) & (X[:, 0] <= shape[0] - 2)
        assert (R[interior] == 2).all() and not R[~interior].any()
        lap = ref.laplacian(par, shape, h, dtype)[0]
        assert abs(float(lap) - 4.0 * interior.sum() / nv) <= 4.0 * ref.U
        # a constant: n = 0 in every cell
        r = ref.reference(np.full(nv, 0.75, np.float32), shape, h, (1.0, 1.0, 1.0), dtype=dtype)
        assert r["terms"][0] == 1 and r["terms"][1] == 0 and r["terms"][2] == 0 and r["V"] == 0 and not r["grad"].any() and np.isfinite(r["loss"])
        # +-c with random signs: every crossing edge adds 2 softplus(k c)
        c, k = 0.3, 5.0
        pm = np.random.default_rng(4).choice(np.array([-c, c], np.float32), nv)
        value, _g, V = ref.sign_vertices(pm, shape, k, dtype)
        kc = k * float(np.float32(c))
        assert V > 0 and abs(float(value) - 2 * (kc + np.log1p(np.exp(-kc)))) <= 1e-5
        assert ref.sign_edges(pm, shape, k, dtype)[1] == V


def test_extent_two_and_boundary_faces_omit_their_axis():
    shape = (2, 4, 3)
    sdf = ref.pure_noise(shape, 5).astype(np.float64)
    R = ref.residual(sdf, shape, (1.0, 1.0, 1.0))
    S = sdf.reshape(3, 4, 2)
    # x has extent 2: only y (interior rows 1, 2) and z (interior plane 1) contribute
    want = np.zeros_like(S)
    want[:, 1:3, :] += (S[:, 0:2, :] - S[:, 1:3, :]) + (S[:, 2:4, :] - S[:, 1:3, :])
    want[1, :, :] += (S[0] - S[1]) + (S[2] - S[1])
    assert np.allclose(R, want, rtol=0, atol=1e-15)
    assert not R[0, 0].any() and not R[2, 3].any()                  # on an edge of the box with x of extent 2: no axis left


def test_no_accuracy_case_sits_on_the_kink(psdr):
    cases = ref.accuracy_cases(psdr.launch_plan_lr((2, 2, 2)).tile)
    assert len(cases) == 24
    for name, shape, sdf in cases:
        assert sdf.dtype == np.float32 and np.isfinite(sdf).all()
        assert ref.kink_margin(sdf, shape, ref.ACCURACY_SPACING) > 1e-3, name
        if name.startswith("noise") or min(shape) >= 7:                  # (the sphere misses every vertex of the smallest lattices: the case V = 0)
            assert ref.crossing_counts(sdf, shape).sum() > 0, name


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
    assert text.index("THE ISOSURFACE") < text.index("THE LATTICE REGULARISERS")
    assert re.search(r"#define\s+PSDR_HIP_ABI_VERSION\s+16\b", text) and L.psdr_hip_abi_version() == 16          # additive: the ABI stays at 16
    for name in ("LatticeRegularizer", "LatregPlan", "lattice_spacing", "launch_plan_lr"):
        assert hasattr(psdr, name)
    names = [u[0] for u in build.hip_units()]
    units = {u[0]: u for u in build.hip_units()}
    assert units["latreg"][1].endswith("latreg.hip") and units["latreg"][1] in build.HIP_SRCS
    assert names.count("latreg") == 1
    assert names.index("sdf") < names.index("mtet") < names.index("latreg") < names.index("pointmesh") and names[-1] == "pointmesh"
    assert names.index("latreg") == names.index("mtet") + 1 == names.index("pointmesh") - 1
    deps = {os.path.relpath(d, ROOT) for d in units["latreg"][3]}
    assert {os.path.join("include", "psdr_hip.h"), os.path.join("psdr_jit_amd", "csrc", "hip", "op_common.h"), os.path.join("psdr_jit_amd", "isa_lint.py")} <= deps
    contract = text[text.index("THE STREAM CONTRACT"):text.index("const char *psdr_hip_last_error")]
    assert all(name in contract for name in NEW)


def test_plan_of_the_python_layer_is_the_librarys(psdr):
    from psdr_jit_amd import cabi
    L = cabi.lib()
    shapes = ((2, 2, 2), (2, 3, 5), (5, 3, 2), (31, 7, 3), (32, 8, 4), (33, 9, 5), (64, 16, 8), (65, 17, 9), (33, 33, 33), (2, 2, 1 << 22), (1 << 22, 2, 2), (2, 1 << 22, 2),
              (256, 256, 256))
    for shape in shapes:
        out = [C.c_int32() for _ in range(5)]
        assert L.psdr_hip_latreg_plan(*shape, *[C.byref(o) for o in out]) == 0
        p = psdr.launch_plan_lr(shape)
        assert [o.value for o in out] == [p.tile[0], p.tile[1], p.tile[2], p.workgroups, p.scratch_floats], shape
        assert (p.num_lattice, p.num_cells) == ref.counts(shape)
        assert p.workgroups == int(np.prod([-(-n // t) for n, t in zip(shape, p.tile)])) and p.scratch_floats == 4 * p.workgroups
    t = psdr.launch_plan_lr((2, 2, 2)).tile
    assert psdr.launch_plan_lr(t).workgroups == 1 and psdr.launch_plan_lr((t[0] + 1, t[1], t[2])).workgroups == 2
    assert psdr.launch_plan_lr((t[0], t[1] + 1, t[2])).workgroups == 2 and psdr.launch_plan_lr((t[0], t[1], t[2] + 1)).workgroups == 2


def test_lattice_spacing_is_that_of_lattice_points(psdr):
    for shape, lo, hi in (((3, 4, 5), -1.0, 1.0), ((12, 11, 10), -1.0, 1.0), ((2, 3, 2), (0.0, -1.0, 2.0), (1.0, 1.5, 2.5))):
        h = psdr.lattice_spacing(shape, lo, hi)
        lo3, hi3 = np.broadcast_to(np.asarray(lo, np.float64), 3), np.broadcast_to(np.asarray(hi, np.float64), 3)
        assert isinstance(h, tuple) and h == tuple(float((hi3[a] - lo3[a]) / (shape[a] - 1)) for a in range(3))
        p = psdr.lattice_points(shape, lo, hi).numpy().astype(np.float64)
        nx, ny = shape[0], shape[1]
        assert abs((p[1, 0] - p[0, 0]) - h[0]) <= 1e-6 and abs((p[nx, 1] - p[0, 1]) - h[1]) <= 1e-6 and abs((p[nx * ny, 2] - p[0, 2]) - h[2]) <= 1e-6
    for bad in (((3, 2, 2), 1.0, 1.0), ((3, 2, 2), 0.0, float("nan")), ((3, 2, 2), (0, 0), 1.0), ((3, 1, 2), 0.0, 1.0)):
        with pytest.raises(ValueError):
            psdr.lattice_spacing(*bad)


def test_the_entry_points_refuse_bad_arguments_before_any_device_call(psdr):
    """no GPU is visible here: a call that reached the device would fail with a HIP error, not with the entry point's own message.  The non-NULL device pointers are host
    addresses that a refused call never reads."""
    from psdr_jit_amd import cabi
    L = cabi.lib()
    host = np.zeros(512, dtype=np.int64)
    p = [host.ctypes.data + 64 * i for i in range(8)]
    one_more = (97, 257, 673)
    assert one_more[0] * one_more[1] * one_more[2] == 2 ** 24 + 1       # Nv = 2^24 + 1 with every extent above 1
    shapes_refused = (((1, 4, 4), "at least 2"), ((4, 1, 4), "at least 2"), ((4, 4, 1), "at least 2"), ((4, 4, 0), "at least 2"), ((-3, 4, 4), "at least 2"),
                      (one_more, "2^24"), ((4097, 4096, 2), "2^24"), ((2 ** 23 + 1, 2, 2), "2^24"), ((2 ** 30, 2 ** 30, 2 ** 30), "2^24"))

    def refused(rc, name, word):
        msg = L.psdr_hip_last_error().decode()
        assert rc != 0 and msg.startswith(name + ":") and word in msg and "hip" not in msg[len(name):].lower(), (name, word, rc, msg)

    name = "psdr_hip_latreg_plan"
    outs = [C.c_int32() for _ in range(5)]
    for shape, word in shapes_refused:
        refused(L.psdr_hip_latreg_plan(*shape, *[C.byref(o) for o in outs]), name, word)
    for k in range(5):
        refused(L.psdr_hip_latreg_plan(4, 4, 4, *[None if i == k else C.byref(o) for i, o in enumerate(outs)]), name, "NULL")
    assert L.psdr_hip_latreg_plan(256, 256, 256, *[C.byref(o) for o in outs]) == 0
    refused(L.psdr_hip_latreg_plan(256, 256, 257, *[C.byref(o) for o in outs]), name, "2^24")

    name = "psdr_hip_latreg_eval"
    keys = ("sdf", "scratch", "out", "crossings", "grad")

    def call(shape=(4, 4, 4), spacing=(0.1, 0.2, 0.3), weights=(1.0, 1.0, 1.0), sign_scale=1.0, **change):
        a = {k: p[i] for i, k in enumerate(keys)}
        a.update(change)
        sp = None if spacing is None else (C.c_double * 3)(*spacing)
        w = None if weights is None else (C.c_float * 3)(*weights)
        return L.psdr_hip_latreg_eval(a["sdf"], *shape, sp, w, sign_scale, a["scratch"], a["out"], a["crossings"], a["grad"], None)

    for shape, word in shapes_refused:
        refused(call(shape=shape), name, word)
    for key in ("sdf", "scratch", "out", "crossings"):
        refused(call(**{key: None}), name, "NULL")
    refused(call(spacing=None), name, "NULL")
    refused(call(weights=None), name, "NULL")
    for bad in ((0.0, 0.2, 0.3), (0.1, -0.2, 0.3), (0.1, 0.2, float("nan")), (float("inf"), 0.2, 0.3), (0.1, 1e-30, 0.3), (1e300, 0.2, 0.3)):
        refused(call(spacing=bad), name, "spacing[")
    for bad in ((-1.0, 1.0, 1.0), (1.0, float("nan"), 1.0), (1.0, 1.0, float("inf"))):
        refused(call(weights=bad), name, "weights[")
    for bad in (-1.0, float("nan"), float("inf")):
        refused(call(sign_scale=bad), name, "sign_scale")
    refused(call(grad=p[0]), name, "of their own")
    refused(call(out=p[0]), name, "of their own")
    refused(call(crossings=p[2]), name, "of their own")
    refused(call(scratch=p[4]), name, "of their own")
    refused(call(grad=None, out=p[1]), name, "of their own")           # the value-only call checks the rest
    assert not host.any()


def test_python_surface_refusals(psdr):
    """wrong arguments are a ValueError before a device is looked for (there is none here)"""
    import torch
    for shape in ((1, 4, 4), (4, 4, 1), (4, 4), (4, 4, 4, 4), (4.0, 4, 4), ("4", 4, 4), None, 4, (True, 4, 4), (97, 257, 673), (257, 65281, 2), (2 ** 24 + 1, 1, 1)):
        with pytest.raises(ValueError):
            psdr.LatticeRegularizer(shape, 0.1)
        with pytest.raises(ValueError):
            psdr.launch_plan_lr(shape)
    assert psdr.LatticeRegularizer((256, 256, 256), 0.1).num_lattice == 2 ** 24
    for spacing in (0.0, -0.1, (0.1, 0.0, 0.1), (0.1, 0.1), float("nan"), float("inf"), "a", None, (0.1, 0.1, -1.0), 1e-30):
        with pytest.raises(ValueError):
            psdr.LatticeRegularizer((3, 4, 5), spacing)
    for weights in ((-1.0, 0.0, 0.0), (1.0, 1.0), (1.0, float("nan"), 0.0), 1.0, None, (1.0, 1.0, float("inf")), ("a", 1, 1)):
        with pytest.raises(ValueError):
            psdr.LatticeRegularizer((3, 4, 5), 0.1, weights=weights)
    for k in (-1.0, float("nan"), float("inf"), "k", None):
        with pytest.raises(ValueError):
            psdr.LatticeRegularizer((3, 4, 5), 0.1, sign_scale=k)
    lr = psdr.LatticeRegularizer((3, 4, 5), (0.1, 0.2, 0.3), weights=(1, 2, 3), sign_scale=2)
    assert lr.shape == (3, 4, 5) and lr.num_lattice == 60 and lr.spacing == (0.1, 0.2, 0.3) and lr.weights == (1.0, 2.0, 3.0) and lr.sign_scale == 2.0
    assert lr.terms is None and lr.num_crossings is None
    assert psdr.LatticeRegularizer((3, 4, 5), 0.5).spacing == (0.5, 0.5, 0.5)
    for bad in (torch.zeros(60, dtype=torch.int32), torch.zeros(59), torch.zeros(61), torch.zeros(60, 1), torch.zeros(5, 4, 3), np.zeros(60, np.int64)):
        for call in (lr, lr.value_and_grad, lr.value):
            with pytest.raises(ValueError):
                call(bad)
    # attributes that a schedule set wrongly are refused at the call, before a device is looked for
    lr.weights = (1.0, -1.0, 0.0)
    with pytest.raises(ValueError):
        lr.value_and_grad(torch.zeros(60))
    lr.weights, lr.sign_scale = (1.0, 0.0, 0.0), -2.0
    with pytest.raises(ValueError):
        lr(torch.zeros(60))
