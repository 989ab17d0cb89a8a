"""GPU tests of the Laplacian vertex preconditioner (psdr_jit_amd/precond.py, csrc/hip/precond.hip): the conjugate-gradient solve and the product with
M = I + lambda L against float64 scipy.sparse on a matrix the tests build themselves, the breakdown guards, bit-for-bit repeatability, both autograd
functions, and the gradient of a rendered image arriving at the differential coordinates.

The bound of the solve is derived, not tuned: lambda_min(M) >= 1 gives |x - x*|_2 <= |b - M x|_2, and the solver stops only when its residual,
recomputed from x, is at most rtol |b|_2."""
import os

import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUNNY = os.path.join(ROOT, "examples", "data", "mesh", "bunny_low.obj")
BALL = os.path.join(scenes.DATA, "cbox_smallball.obj")
RTOL = 1e-4
U = 2.0 ** -24


@pytest.fixture(scope="module")
def psdr():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists)")
    import __graft_entry__
    __graft_entry__.build()
    import psdr_jit_amd
    return psdr_jit_amd


def _obj(psdr, path):
    m = psdr.Mesh()
    m.load(path)
    return np.asarray(m.face_indices).reshape(-1, 3).astype(np.int64), int(m.num_vertices)


def _grid(m):
    idx = np.arange(m * m).reshape(m, m)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    return np.concatenate([np.stack([a, b, d], 1), np.stack([a, d, c], 1)]), m * m


def _fan(k):
    """k triangles round hub 0, rim 1..k, and vertex k + 1 that no face uses"""
    return np.array([[0, 1 + i, 1 + (i + 1) % k] for i in range(k)]), k + 2


def _mesh(psdr, name):
    if name == "tetrahedron":
        return np.array([[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]]), 4, 19.0
    if name == "ball":
        return _obj(psdr, BALL) + (19.0,)
    if name == "bunny":
        return _obj(psdr, BUNNY) + (19.0,)
    if name == "grid":
        return _grid(257) + (19.0,)
    return _fan(200) + (1.0,)


def _matrix(faces, n, lam):
    """M in float64, from the faces alone (not through laplacian_csr)"""
    import scipy.sparse as sp
    f = np.asarray(faces)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2], f[:, 1], f[:, 2], f[:, 0]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0], f[:, 0], f[:, 1], f[:, 2]])
    A = sp.coo_matrix((np.ones(len(a)), (a, b)), shape=(n, n)).tocsr()
    A.data[:] = 1.0                     # an edge counts once, however many faces share it
    A.setdiag(0.0)
    A.eliminate_zeros()
    deg = np.asarray(A.sum(axis=1)).ravel()
    return (sp.identity(n) + lam * (sp.diags(deg) - A)).tocsc()


_CACHE = {}


def _setup(psdr, name):
    """(preconditioner, M, n) per mesh, built once"""
    if name not in _CACHE:
        faces, n, lam = _mesh(psdr, name)
        _CACHE[name] = (psdr.LaplacianPreconditioner(faces, n, lambda_=lam, rtol=RTOL), _matrix(faces, n, lam), n)
    return _CACHE[name]


def _spsolve(M, b):
    from scipy.sparse.linalg import spsolve
    return np.stack([spsolve(M, np.asarray(b, np.float64)[:, c]) for c in range(3)], 1)


def _check_solution(x, M, b, label):
    """per column: finite, and |x - x*|_2 <= rtol |b|_2"""
    x = np.asarray(x, np.float64)
    assert np.isfinite(x).all(), label
    err = np.linalg.norm(x - _spsolve(M, b), axis=0)
    bound = RTOL * np.linalg.norm(np.asarray(b, np.float64), axis=0)
    print(label, "|x - x*|", err, "rtol |b|", bound)
    assert np.all(err <= bound), (label, err, bound)


@pytest.mark.parametrize("name", ["tetrahedron", "ball", "bunny", "grid", "fan"])
def test_solve_matches_float64(psdr, name):
    import torch
    pre, M, n = _setup(psdr, name)
    if name == "ball":
        assert n == 162
    if name == "bunny":
        assert n == 2503
    if name == "grid":
        assert n == 66049 and (n + 255) // 256 > 256
    if name == "fan":
        deg = np.diff(pre.row_begin)
        assert n == 202 and deg[0] == 200 and deg[-1] == 0
    b = np.random.default_rng(5).standard_normal((n, 3)).astype(np.float32)
    x = pre.from_differential(torch.from_numpy(b))
    assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (n, 3)
    info = pre.last_solve
    print(name, info)
    assert info["converged"] and 0 < info["iterations"] <= pre.max_iter
    assert all(r <= RTOL for r in info["rel_residual"])
    _check_solution(x.cpu().numpy(), M, b, name)


def test_guards_zero_column_and_scaled_column(psdr):
    import torch
    pre, M, n = _setup(psdr, "ball")
    b = np.random.default_rng(6).standard_normal((n, 3)).astype(np.float32)
    b[:, 1] = 0.0
    b[:, 2] = np.float32(1e6) * b[:, 0]
    x = pre.from_differential(torch.from_numpy(b)).cpu().numpy()
    assert pre.last_solve["converged"]
    assert not np.isnan(x).any()
    assert np.all(x[:, 1] == 0.0) and not np.any(np.signbit(x[:, 1])), "a zero right-hand side must give exactly zero"
    _check_solution(x[:, [0, 2, 2]], M, b[:, [0, 2, 2]], "guards")
    # a solve that cannot converge says so, with the residuals
    short = psdr.LaplacianPreconditioner(*_mesh(psdr, "bunny")[:2], lambda_=19.0, rtol=RTOL, max_iter=3)
    with pytest.raises(RuntimeError, match="no convergence"):
        short.from_differential(torch.ones(short.num_vertices, 3))
    assert short.last_solve["iterations"] == 3 and not short.last_solve["converged"]


def _apply_bound(pre, lam, x):
    """gamma_k ((1 + lam deg_i) |x_i| + lam sum_j |x_j|), k = deg_i + 3: the standard bound of the row's float32 sum"""
    import scipy.sparse as sp
    n = pre.num_vertices
    A = sp.csr_matrix((np.ones(len(pre.col)), pre.col, pre.row_begin), shape=(n, n))
    deg = np.diff(pre.row_begin).astype(np.float64)
    ax = np.abs(np.asarray(x, np.float64))
    k = deg + 3.0
    gamma = k * U / (1.0 - k * U)
    return gamma[:, None] * ((1.0 + lam * deg)[:, None] * ax + lam * (A @ ax))


@pytest.mark.parametrize("name", ["bunny", "fan"])
def test_apply_within_the_summation_bound(psdr, name):
    import torch
    pre, M, n = _setup(psdr, name)
    x = np.random.default_rng(7).standard_normal((n, 3)).astype(np.float32)
    y = pre.to_differential(torch.from_numpy(x))
    assert y.is_cuda and tuple(y.shape) == (n, 3)
    want = M @ x.astype(np.float64)
    err, bound = np.abs(y.cpu().numpy().astype(np.float64) - want), _apply_bound(pre, pre.lambda_, x)
    print(name, "worst error / bound", float((err / np.maximum(bound, 1e-300)).max()))
    assert np.all(err <= bound)
    assert np.abs(want).max() > 1.0


def test_solve_is_deterministic(psdr):
    import torch
    pre, M, n = _setup(psdr, "grid")
    rng = np.random.default_rng(8)
    b1, b2 = (torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32)).cuda() for _ in range(2))
    x1 = pre.from_differential(b1).clone()
    it1 = pre.last_solve["iterations"]
    x2 = pre.from_differential(b2).clone()
    x3 = pre.from_differential(b1).clone()
    assert pre.last_solve["iterations"] == it1
    assert torch.equal(x1, x3)
    assert not torch.equal(x1, x2)


def test_autograd_of_both_directions(psdr):
    import torch
    pre, M, n = _setup(psdr, "bunny")
    rng = np.random.default_rng(9)
    w = rng.standard_normal((n, 3)).astype(np.float32)
    wt = torch.from_numpy(w).cuda()
    # the backward of the solve is a solve
    u = torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32)).requires_grad_()
    (wt * pre.from_differential(u)).sum().backward()
    assert u.grad is not None and u.grad.device == u.device and tuple(u.grad.shape) == (n, 3)
    err = np.linalg.norm(u.grad.numpy().astype(np.float64) - _spsolve(M, w), axis=0)
    bound = RTOL * np.linalg.norm(w.astype(np.float64), axis=0)
    print("solve backward", err, bound)
    assert np.all(err <= bound)
    # the backward of the product is the product
    v = torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32)).cuda().requires_grad_()
    (wt * pre.to_differential(v)).sum().backward()
    err = np.abs(v.grad.cpu().numpy().astype(np.float64) - M @ w.astype(np.float64))
    assert np.all(err <= _apply_bound(pre, pre.lambda_, w))
    # there and back
    V = rng.standard_normal((n, 3)).astype(np.float32)
    back = pre.from_differential(pre.to_differential(torch.from_numpy(V))).cpu().numpy().astype(np.float64)
    err = np.linalg.norm(back - V.astype(np.float64), axis=0)
    bound = RTOL * np.linalg.norm(M @ V.astype(np.float64), axis=0)
    print("round trip", err, bound)
    assert np.all(err <= bound)


def test_gradient_of_a_render_reaches_the_differential_coordinates(psdr):
    """the scene of test_reverse_mode_through_vertex_normals: the ball's vertices are M^-1 u, and u.grad = M^-1 v.grad from ONE render"""
    import torch
    from psdr_jit_amd import Matrix4fC, Matrix4fD
    D = scenes.DATA
    sc = psdr.Scene()
    sc.opts.spp, sc.opts.sppe, sc.opts.sppse = 8, 8, 8
    sc.opts.width = sc.opts.height = 40
    sc.opts.log_level = 0
    cam = psdr.PerspectiveCamera(60, 0.000001, 10000000.)
    cam.to_world = Matrix4fD([[1., 0., 0., 278.], [0., 1., 0., 273.], [0., 0., 1., -500.], [0., 0., 0., 1.]])
    sc.add_Sensor(cam)
    sc.add_BSDF(psdr.DiffuseBSDF([0.0, 0.0, 0.0]), "light")
    sc.add_BSDF(psdr.DiffuseBSDF([0.9, 0.6, 0.1]), "ball")
    sc.add_BSDF(psdr.DiffuseBSDF([0.95, 0.95, 0.95]), "white")
    I = np.eye(4, dtype=np.float32).tolist()
    sc.add_Mesh(os.path.join(D, "cbox_luminaire.obj"), Matrix4fC([[1., 0., 0., 0.], [0., 1., 0., -0.5], [0., 0., 1., 0.], [0., 0., 0., 1.]]), "light", psdr.AreaLight([20.0, 20.0, 8.0]))
    ball = psdr.Mesh()
    ball.load(os.path.join(D, "cbox_smallball.obj"))
    V0 = torch.tensor(np.asarray(ball.vertex_positions, np.float32))
    pre = psdr.LaplacianPreconditioner(ball, lambda_=19.0, rtol=RTOL)
    u = pre.to_differential(V0).detach().requires_grad_()
    v = pre.from_differential(u)
    v.retain_grad()
    ball.vertex_positions = v
    sc.add_Mesh(ball, "ball", None)
    for f in ("cbox_floor", "cbox_back"):
        sc.add_Mesh(os.path.join(D, f + ".obj"), Matrix4fC(I), "white", None)
    sc.configure()
    sc.configure([0])
    img = psdr.PathTracer(2).renderD(sc, 0, seed=9)
    w = torch.linspace(0.5, 1.5, img.numel(), device=img.device).reshape(img.shape)
    (img * w).sum().backward()
    assert v.grad is not None and u.grad is not None
    gv = v.grad.cpu().numpy().astype(np.float64)
    assert np.isfinite(gv).all() and np.all(np.linalg.norm(gv, axis=0) > 0.0)
    M = _matrix(np.asarray(ball.face_indices).reshape(-1, 3), int(ball.num_vertices), 19.0)
    err = np.linalg.norm(u.grad.cpu().numpy().astype(np.float64) - _spsolve(M, gv), axis=0)
    bound = RTOL * np.linalg.norm(gv, axis=0)
    print("u.grad", err, bound)
    assert np.all(err <= bound)
