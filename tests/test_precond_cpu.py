"""The Laplacian vertex preconditioner, what can be checked without a GPU: the four entry points are declared, exported and listed, the ABI version did
not move, psdr_hip_precond_create refuses bad lists before it touches a device, laplacian_csr builds the pattern of the matrix an independent
scipy.sparse construction gives, and AdamUniform takes the steps of its formulas evaluated in float64."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("psdr_hip_precond_create", "psdr_hip_precond_apply", "psdr_hip_precond_solve", "psdr_hip_precond_destroy")
BUNNY = os.path.join(ROOT, "examples", "data", "mesh", "bunny_low.obj")


@pytest.fixture(scope="module")
def psdr():
    import __graft_entry__
    __graft_entry__.build()
    import psdr_jit_amd
    return psdr_jit_amd


def test_entry_points_declared_exported_listed(psdr):
    from psdr_jit_amd import cabi
    with open(os.path.join(ROOT, "include", "psdr_hip.h")) as fh:
        text = fh.read()
    L = cabi.lib()
    for name in NEW:
        assert re.search(r"^int\s+%s\s*\(" % name, text, re.M), "%s is not declared in include/psdr_hip.h" % name
        assert hasattr(L, name), "libpsdr_hip.so does not export %s" % name
        assert name in cabi.SYMBOLS
    assert re.search(r"typedef struct psdr_precond_info \{", text)
    assert re.search(r"#define\s+PSDR_HIP_ABI_VERSION\s+16\b", text)
    assert L.psdr_hip_abi_version() == 16
    for name in ("laplacian_csr", "LaplacianPreconditioner", "AdamUniform"):
        assert hasattr(psdr, name)


def _create(L, n, row_begin, col, lam=19.0):
    rb = np.asarray(row_begin, np.int32) if row_begin is not None else None
    cl = np.asarray(col, np.int32) if col is not None else None
    h = C.c_void_p()
    rc = L.psdr_hip_precond_create(n, rb.ctypes.data if rb is not None else None, cl.ctypes.data if cl is not None else None, lam, C.byref(h), None)
    return rc, h, L.psdr_hip_last_error().decode()


def test_create_refuses_bad_lists_before_any_device_call(psdr):
    from psdr_jit_amd import cabi
    L = cabi.lib()
    good_rb, good_col = [0, 1, 2], [1, 0]
    cases = [
        ("NULL", 2, None, good_col), ("NULL", 2, good_rb, None),
        ("positive", 0, good_rb, good_col), ("positive", -3, good_rb, good_col),
        ("row_begin[0]", 2, [1, 1, 2], good_col),
        ("monotonic", 3, [0, 2, 1, 2], [1, 0]),
        ("outside", 2, good_rb, [2, 0]), ("outside", 2, good_rb, [1, -1]),
        ("itself", 2, good_rb, [0, 0]),
    ]
    for word, n, rb, col in cases:
        rc, h, msg = _create(L, n, rb, col)
        assert rc != 0 and not h.value, (word, n, rb, col)
        assert "psdr_hip_precond_create" in msg and word in msg, (word, msg)
    rb, col = np.asarray(good_rb, np.int32), np.asarray(good_col, np.int32)
    assert L.psdr_hip_precond_create(2, rb.ctypes.data, col.ctypes.data, 19.0, None, None) != 0
    rc, h, msg = _create(L, 2, good_rb, good_col, lam=float("nan"))
    assert rc != 0 and "lambda" in msg
    # the other calls refuse null arguments as well
    info = cabi.PrecondInfo()
    assert L.psdr_hip_precond_apply(None, None, None, None) != 0
    assert L.psdr_hip_precond_solve(None, None, None, 1e-4, 10, C.byref(info), None) != 0
    assert L.psdr_hip_precond_destroy(None) != 0
    assert "NULL" in L.psdr_hip_last_error().decode()


def _reference_matrix(faces, n, lam):
    """M = I + lam (D - A), built without laplacian_csr: a dictionary-of-keys adjacency filled edge by edge"""
    import scipy.sparse as sp
    A = sp.dok_matrix((n, n), dtype=np.float64)
    for f in np.asarray(faces).reshape(-1, 3):
        for a, b in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0])):
            if a != b:
                A[int(a), int(b)] = 1.0
                A[int(b), int(a)] = 1.0
    A = A.tocsr()
    deg = np.asarray(A.sum(axis=1)).ravel()
    return (sp.identity(n) + lam * (sp.diags(deg) - A)).tocsr()


def _matrix_of(row_begin, col, lam):
    import scipy.sparse as sp
    n = len(row_begin) - 1
    A = sp.csr_matrix((np.ones(len(col)), col, row_begin), shape=(n, n))
    return (sp.identity(n) + lam * (sp.diags(np.diff(row_begin).astype(np.float64)) - A)).tocsr()


def _bunny(psdr):
    m = psdr.Mesh()
    m.load(BUNNY)
    return np.asarray(m.face_indices).reshape(-1, 3), int(m.num_vertices)


def _cases(psdr):
    yield ("bunny",) + _bunny(psdr)
    yield "three faces on one edge", [[0, 1, 2], [0, 1, 3], [1, 0, 4]], 5
    yield "duplicated face", [[0, 1, 2], [0, 1, 2], [2, 1, 3]], 4
    yield "face (i, i, j)", [[0, 1, 2], [3, 3, 1]], 4
    yield "isolated vertex", [[0, 1, 2], [2, 1, 4]], 6


def test_laplacian_csr_matches_an_independent_construction(psdr):
    lam = 19.0
    seen = set()
    for name, faces, n in _cases(psdr):
        rb, col = psdr.laplacian_csr(faces, n)
        assert rb.dtype == np.int32 and col.dtype == np.int32 and rb.shape == (n + 1,) and rb[0] == 0 and rb[-1] == len(col), name
        assert np.all(np.diff(rb) >= 0), name
        rows = np.repeat(np.arange(n), np.diff(rb))
        assert not np.any(rows == col), name + ": self-loop"
        for i in range(n):
            c = col[rb[i]:rb[i + 1]]
            assert np.all(np.diff(c) > 0), name + ": columns of row %d are not sorted and distinct" % i
        pairs = set(zip(rows.tolist(), col.tolist()))
        assert pairs == {(b, a) for a, b in pairs}, name + ": the pattern is not symmetric"
        M, want = _matrix_of(rb, col, lam), _reference_matrix(faces, n, lam)
        assert abs(M - want).max() == 0.0, name
        assert np.array_equal(np.asarray(M.sum(axis=1)).ravel(), np.ones(n)), name + ": the rows of M do not sum to 1"
        seen.add(name)
        if name == "bunny":
            deg = np.diff(rb)
            assert n == 2503 and deg.min() == 3 and deg.max() == 10
        if name == "three faces on one edge":
            assert col[rb[0]:rb[1]].tolist() == [1, 2, 3, 4] and col[rb[1]:rb[2]].tolist() == [0, 2, 3, 4]
        if name == "face (i, i, j)":
            assert col[rb[3]:rb[4]].tolist() == [1]
        if name == "isolated vertex":
            assert rb[4] == rb[3] and rb[6] == rb[5]
    assert len(seen) == 5


def test_adam_uniform_follows_its_formulas(psdr):
    import torch
    rng = np.random.default_rng(11)
    p0 = rng.standard_normal((7, 3))
    grads = [rng.standard_normal((7, 3)) * s for s in (1.0, 0.1, 5.0)]
    lr, b1, b2 = 0.05, 0.9, 0.999
    p = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = psdr.AdamUniform([p], lr=lr, betas=(b1, b2))
    want, m1, m2 = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    for t, g in enumerate(grads, 1):
        p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        m1 = b1 * m1 + (1 - b1) * g
        m2 = b2 * m2 + (1 - b2) * g * g
        want = want - lr * (m1 / (1 - b1 ** t)) / np.sqrt(m2 / (1 - b2 ** t)).max()
        # float64 on both sides: a handful of roundings per element
        assert np.abs(p.detach().numpy() - want).max() <= 1e-14 * max(1.0, np.abs(want).max()), t
    # one denominator per tensor: the first step moves every coordinate by lr * g / max|g|
    q = torch.zeros(4, dtype=torch.float64, requires_grad=True)
    opt = psdr.AdamUniform([q], lr=1.0)
    q.grad = torch.tensor([1.0, -2.0, 0.5, 0.0], dtype=torch.float64)
    opt.step()
    assert np.allclose(q.detach().numpy(), [-0.5, 1.0, -0.25, 0.0], rtol=1e-12, atol=0)
    # a zero gradient leaves the tensor where it is (no 0 / 0)
    z = torch.ones(3, requires_grad=True)
    opt = psdr.AdamUniform([z], lr=0.1)
    z.grad = torch.zeros(3)
    opt.step()
    assert torch.equal(z.detach(), torch.ones(3))
