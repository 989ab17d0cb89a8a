"""Laplacian vertex preconditioner ("Large Steps in Inverse Rendering", Nicolet et al. 2021) on the GPU.

A per-vertex gradient from a path tracer is noisy and concentrated on silhouettes; a few optimiser steps on it tangle the mesh.
The recipe re-parametrises the vertices through M = I + lambda L (L the combinatorial Laplacian of the mesh): it optimises
u = M v, renders v = M^-1 u, and the gradient that reaches u is M^-1 dloss/dv - a smooth descent direction.

    pre = psdr.LaplacianPreconditioner(mesh, lambda_=19.0)
    u = pre.to_differential(V0).detach().requires_grad_()
    opt = psdr.AdamUniform([u], lr=...)
    # each step:
    mesh.vertex_positions = pre.from_differential(u); sc.configure()
    loss(renderD(...)).backward(); opt.step()

Both directions run in libpsdr_hip.so (psdr_hip_precond_apply / psdr_hip_precond_solve, csrc/hip/precond.hip): the product with M is one
kernel, the solve a Jacobi-preconditioned conjugate-gradient iteration of plain launches on torch's current stream.
"""
import ctypes as _C

import numpy as _np
import torch as _torch

from . import cabi as _cabi


def laplacian_csr(faces, num_vertices):
    """CSR pattern (row_begin [n + 1], col [nnz], int32) of the combinatorial Laplacian of a triangle list: the distinct undirected
    edges of `faces` ([f, 3] vertex ids) in both directions, columns sorted per row.  A face with a repeated index adds no self-loop,
    an edge shared by any number of faces counts once, a vertex no face uses has an empty row.  Host-side, run once per mesh."""
    n = int(num_vertices)
    if n <= 0:
        raise ValueError("laplacian_csr: num_vertices must be positive")
    f = _np.asarray(faces)
    if f.size == 0:
        f = _np.zeros((0, 3), dtype=_np.int64)
    if f.ndim != 2 or f.shape[1] != 3:
        raise ValueError("laplacian_csr: faces must be [f, 3]")
    f = f.astype(_np.int64)
    if f.size and (f.min() < 0 or f.max() >= n):
        raise ValueError("laplacian_csr: a face index is outside [0, %d)" % n)
    a = _np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = _np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    keep = a != b
    a, b = a[keep], b[keep]
    key = _np.unique(_np.concatenate([a * n + b, b * n + a]))          # sorted by row, then by column; duplicates gone
    row, col = key // n, key % n
    row_begin = _np.zeros(n + 1, dtype=_np.int64)
    _np.cumsum(_np.bincount(row, minlength=n), out=row_begin[1:])
    if row_begin[-1] >= 2 ** 31:
        raise ValueError("laplacian_csr: more than 2^31 - 1 entries")
    return row_begin.astype(_np.int32), col.astype(_np.int32)


class _Handle:
    """owner of a psdr_hip_precond"""

    def __init__(self, row_begin, col, lambda_, stream):
        self.ptr = _C.c_void_p()
        rb, cl = _np.ascontiguousarray(row_begin, _np.int32), _np.ascontiguousarray(col, _np.int32)
        _cabi.check(_cabi.lib().psdr_hip_precond_create(int(rb.size - 1), rb.ctypes.data, cl.ctypes.data if cl.size else None, float(lambda_),
                                                        _C.byref(self.ptr), stream))

    def __del__(self):
        if getattr(self, "ptr", None) and _cabi is not None:           # (None: the interpreter is shutting down and has cleared the module)
            _cabi.lib().psdr_hip_precond_destroy(self.ptr)
            self.ptr = None


def _on_device(t, n, dev):
    if tuple(t.shape) != (n, 3):
        raise ValueError("expected a [%d, 3] tensor, got %s" % (n, tuple(t.shape)))
    return t.detach().to(dev, _torch.float32).contiguous()


class _ApplyFn(_torch.autograd.Function):
    """y = M x; M is symmetric, so the adjoint is the same product"""

    @staticmethod
    def forward(ctx, pre, x):
        ctx.pre, ctx.like = pre, (x.device, x.dtype)
        return pre._apply(x)

    @staticmethod
    def backward(ctx, g):
        return None, ctx.pre._apply(g).to(*ctx.like)


class _SolveFn(_torch.autograd.Function):
    """x = M^-1 b; the adjoint is another solve"""

    @staticmethod
    def forward(ctx, pre, b):
        ctx.pre, ctx.like = pre, (b.device, b.dtype)
        return pre._solve(b)

    @staticmethod
    def backward(ctx, g):
        return None, ctx.pre._solve(g).to(*ctx.like)


class LaplacianPreconditioner:
    """M = I + lambda_ L for one mesh, L the combinatorial Laplacian (degree on the diagonal, -1 per distinct edge).

    mesh_or_faces: a Mesh (its face_indices and num_vertices are read) or a [f, 3] array of vertex ids with `num_vertices`.
    There is no vertex welding: positions an OBJ file lists twice are two vertices here, and a seam between them is a boundary
    of the Laplacian (its two sides move apart under a large lambda_).  Weld the mesh before it is loaded where that matters.

    to_differential(v) = M v and from_differential(u) = M^-1 u take a float32 [n, 3] tensor on any device and return one on the
    render device, computed on torch's current stream; both are differentiable (M is symmetric: the backward of the product is
    the product, the backward of the solve is a solve).  `last_solve` is the record of the most recent solve: iterations,
    converged, launches, rel_residual (per column |b - M x|_2 / |b|_2, from the residual recomputed from x).  A solve that does
    not reach rtol within max_iter iterations raises RuntimeError with the residuals.

    rtol: the solve stops when every column's recomputed residual is at most rtol |b|_2.  The default rests on float32: the worst-case
    attainable relative residual is about 2^-24 (1 + 2 lambda deg_max), which is 2.3e-5 for lambda = 19 at degree 10, which is why
    1e-5 is not the default.
    """

    def __init__(self, mesh_or_faces, num_vertices=None, lambda_=19.0, rtol=1e-4, max_iter=1000):
        from . import _device, _stream_ptr
        if hasattr(mesh_or_faces, "face_indices") and hasattr(mesh_or_faces, "num_vertices"):
            faces = _np.asarray(mesh_or_faces.face_indices).reshape(-1, 3)
            num_vertices = int(mesh_or_faces.num_vertices) if num_vertices is None else int(num_vertices)
        else:
            faces = _np.asarray(mesh_or_faces).reshape(-1, 3)
            if num_vertices is None:
                raise ValueError("LaplacianPreconditioner: num_vertices is required with a face array")
        self.num_vertices = int(num_vertices)
        self.lambda_, self.rtol, self.max_iter = float(lambda_), float(rtol), int(max_iter)
        self.row_begin, self.col = laplacian_csr(faces, self.num_vertices)
        self.last_solve = None
        self._device = _device()
        with _torch.cuda.device(self._device):
            self._handle = _Handle(self.row_begin, self.col, self.lambda_, _stream_ptr())

    def _apply(self, x):
        from . import _stream_ptr
        x = _on_device(x, self.num_vertices, self._device)
        y = _torch.empty_like(x)
        _cabi.check(_cabi.lib().psdr_hip_precond_apply(self._handle.ptr, x.data_ptr(), y.data_ptr(), _stream_ptr()))
        return y

    def _solve(self, b):
        from . import _stream_ptr
        b = _on_device(b, self.num_vertices, self._device)
        x = _torch.empty_like(b)
        info = _cabi.PrecondInfo()
        _cabi.check(_cabi.lib().psdr_hip_precond_solve(self._handle.ptr, b.data_ptr(), x.data_ptr(), self.rtol, self.max_iter, _C.byref(info), _stream_ptr()))
        self.last_solve = {"iterations": int(info.iterations), "converged": bool(info.converged), "launches": int(info.launches),
                           "rel_residual": tuple(float(v) for v in info.rel_residual)}
        if not info.converged:
            raise RuntimeError("LaplacianPreconditioner: no convergence to rtol = %g in %d iterations; |b - M x| / |b| per column = %s"
                               % (self.rtol, info.iterations, self.last_solve["rel_residual"]))
        return x

    def to_differential(self, v):
        """u = M v"""
        return _ApplyFn.apply(self, v)

    def from_differential(self, u):
        """v = M^-1 u"""
        return _SolveFn.apply(self, u)


class AdamUniform(_torch.optim.Optimizer):
    """Adam with ONE denominator per tensor (Nicolet et al. 2021): per-coordinate Adam rescales every coordinate by its own gradient
    history, which undoes the isotropy the preconditioner gives the step.

        m1 <- b1 m1 + (1 - b1) g,   m2 <- b2 m2 + (1 - b2) g^2
        p  <- p - lr (m1 / (1 - b1^t)) / max(sqrt(m2 / (1 - b2^t)))        the max over all elements of the tensor

    A tensor whose gradients have all been zero so far is left where it is."""

    def __init__(self, params, lr, betas=(0.9, 0.999)):
        if not lr > 0.0:
            raise ValueError("AdamUniform: lr must be positive")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("AdamUniform: betas must lie in [0, 1)")
        super().__init__(params, dict(lr=lr, betas=tuple(betas)))

    @_torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with _torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            lr, (b1, b2) = group["lr"], group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = p.grad
                st = self.state[p]
                if not st:
                    st["step"], st["m1"], st["m2"] = 0, _torch.zeros_like(p), _torch.zeros_like(p)
                st["step"] += 1
                t = st["step"]
                st["m1"].mul_(b1).add_(g, alpha=1.0 - b1)
                st["m2"].mul_(b2).addcmul_(g, g, value=1.0 - b2)
                denom = (st["m2"] / (1.0 - b2 ** t)).sqrt().max()
                # all gradients zero so far: m1 is zero too, and the step is 0 / tiny = 0
                p.addcdiv_(st["m1"] / (1.0 - b1 ** t), denom.clamp_min(_torch.finfo(p.dtype).tiny), value=-lr)
        return loss
