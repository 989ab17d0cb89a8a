"""The Chamfer distance between two point sets, value and both gradients, and the sampling of points from a mesh's surface (kernels:
csrc/hip/chamfer.hip).

The image losses and the mesh regularisers measure the image and the mesh's smoothness; this measures the shape itself - how far a fitted mesh is from a target shape, a
scan or a point cloud (pytorch3d's sample_points_from_meshes and chamfer_distance are the ones users know):

    sam, cd = psdr.SurfaceSampler(mesh, num_points=20000), psdr.ChamferDistance()
    sam.resample(V0)                                                    # every k steps: sam.resample(v.detach())
    loss = ms(img, target) + reg(v) + 0.1 * cd(sam(v), target_points)   # target_points: a scan, or SurfaceSampler(target_mesh)(Vt)

The definition (include/psdr_hip.h states it in full).  x [N, 3], y [M, 3], float32, 1 <= N, M <= 2^26, finite.
    d2(i, j)  = (dx dx + dy dy) + dz dz,  dx = x_i0 - y_j0 ...          the difference form, every operation one float32 rounding: no cancellation, and bit for bit
                                                                        what a numpy float32 statement gives
    a(i)      = the lowest j that minimises d2(i, j), dist2_xy[i] = d2(i, a(i));  b(j), dist2_yx[j] the same with the roles swapped
    loss      = w_xy (1 / N) sum_i rho(dist2_xy[i]) + w_yx (1 / M) sum_j rho(dist2_yx[j])      rho(s) = s (squared=True) or sqrt(s), with derivative 0 at s = 0;
                                                                        a term of weight 0 is not evaluated
    gradient  the indices are constants: x_i receives its own term's and, through an inverted index of b built on the device at every call (a stable sort), those of the
              y_j that chose it, in ascending j; y_j the mirror image
Written in torch ops, cdist(x, y).min() materialises an N x M matrix and uses the expansion |x|^2 + |y|^2 - 2 x.y, which cancels where a neighbour is near, and its
backward scatters with float atomics.  Here the scan keeps the queries in registers and streams the candidates through LDS, nothing of size N x M exists, there are no
float atomics and no host synchronisation, and the same inputs give the same bits.

For large clouds the same neighbours, bit for bit, come from a uniform grid over the candidates instead of the scan (pointgrid.py):
nearest_points(x, y, search="grid"), nearest_points(x, PointGrid(y)), ChamferDistance(search="grid"), cd(x, y, y_grid=grid).  The default stays "scan".

launch_plan(n, m) is the scan's split into query blocks x candidate slices, which psdr_hip_chamfer_plan states in C; the result does not depend on it.
SurfaceSampler draws its points on the host (numpy, once per resample) and applies them on the GPU as a sparse matrix through the subdivision operator's kernels.  One GPU
only: under an initialised torch.distributed group of more than one rank the calls raise."""
import collections as _collections
import ctypes as _C
import math as _math

import functools as _functools

import numpy as _np

from . import pointgrid as _pg
from ._opcommon import MAX_COUNT, NARROW_MAX, TARGET_GROUPS, SCAN_THREADS as THREADS, _ceil_div, _checked_points, _faces_checked, _inverted, _single_gpu, slice_plan  # noqa: F401

TILE = 1024                  # candidates per LDS tile
WIDE_QUERIES = 4             # queries per lane for n > NARROW_MAX, else 1

LaunchPlan = _collections.namedtuple("LaunchPlan", ["tile", "queries_per_lane", "slices", "slice_len"])


def launch_plan(n, m):
    """How the scan of n queries over m candidates is split: LaunchPlan(tile, queries_per_lane, slices, slice_len), a pure function (csrc/hip/chamfer.hip: plan_of).

    A workgroup holds 256 queries_per_lane queries; slice s holds the candidates [s slice_len, min(m, (s + 1) slice_len)); the grid is query blocks x slices."""
    n, m = int(n), int(m)
    return LaunchPlan(*slice_plan(n, m, TILE, WIDE_QUERIES, "launch_plan: n = %d, m = %d, both must lie in [1, 2^26]" % (n, m)))


def _checked_weights(weights):
    try:
        w = tuple(float(x) for x in weights)
    except (TypeError, ValueError):
        raise ValueError("ChamferDistance: weights must be two numbers (x -> y, y -> x), got %r" % (weights,)) from None
    if len(w) != 2 or not all(_math.isfinite(x) and x >= 0.0 for x in w):
        raise ValueError("ChamferDistance: weights must be two finite numbers >= 0 (x -> y, y -> x), got %r" % (weights,))
    return w


def _nearest(x, y, device):
    """x, y: float32 contiguous on `device` -> (index int32 [N], dist2 float32 [N]) on the current stream"""
    import torch
    from . import cabi, _stream_ptr
    n, m = int(x.shape[0]), int(y.shape[0])
    keys = torch.empty(n, device=device, dtype=torch.int64)
    index = torch.empty(n, device=device, dtype=torch.int32)
    dist2 = torch.empty(n, device=device, dtype=torch.float32)
    cabi.check(cabi.lib().psdr_hip_chamfer_nearest(x.data_ptr(), n, y.data_ptr(), m, keys.data_ptr(), index.data_ptr(), dist2.data_ptr(), _stream_ptr()))
    return index, dist2


def nearest_points(x, y, search="scan", return_stats=False):
    """For every x_i the lowest index j of its nearest y_j and the squared distance: (index int32 [N], dist2 float32 [N]) on the render device, detached, computed on
    torch's current stream without a host synchronisation.  x [N, 3], y [M, 3] on any device and of any float dtype; the distance is the module docstring's d2, bit for
    bit.

    search: "scan" (the default: the brute-force scan) or "grid": a uniform grid of y is built and searched (pointgrid.py), which returns the same bits.  y may be a
    PointGrid built earlier; that grid is searched, whatever `search` says.  return_stats=True (grid searches only) adds a third value, an int64 [2] device tensor: the
    queries that the fallback pass finished, and the (query, candidate) pairs tested."""
    _pg._checked_search(search, "nearest_points")
    x = _checked_points(x, "nearest_points", "x")
    grid = _pg._checked_grid(y, "nearest_points", "y") if isinstance(y, _pg.PointGrid) else None
    if grid is None:
        y = _checked_points(y, "nearest_points", "y")
        if return_stats and search != "grid":
            raise ValueError("nearest_points: return_stats needs search=\"grid\" or a PointGrid")
    _single_gpu("nearest_points")
    import torch
    from . import _device
    device = _device()
    with torch.cuda.device(device):
        x = x.detach().to(device, torch.float32).contiguous()
        if grid is None and search == "scan":
            return _nearest(x, y.detach().to(device, torch.float32).contiguous(), device)
        if grid is None:
            grid = _pg.PointGrid(y)
        _pg._on_render_device(grid, device, "nearest_points", "y")
        index, dist2, stats = _pg._grid_nearest(x, grid, device, return_stats)
    return (index, dist2, stats) if return_stats else (index, dist2)


@_functools.lru_cache(maxsize=None)
def _fns():
    import torch

    class _ChamferFn(torch.autograd.Function):
        """cd(x, y): the forward also produces both gradients, the backward scales them by the incoming scalar"""

        @staticmethod
        def forward(ctx, cd, x, y, y_grid):
            out, gx, gy = cd._eval(x, y, True, y_grid)
            ctx.save_for_backward(gx, gy)
            ctx.like = ((x.device, x.dtype), (y.device, y.dtype))
            return out[0]

        @staticmethod
        def backward(ctx, g):
            gx, gy = ctx.saved_tensors
            return None, (g * gx).to(*ctx.like[0]) if ctx.needs_input_grad[1] else None, (g * gy).to(*ctx.like[1]) if ctx.needs_input_grad[2] else None, None

    class _SampleFn(torch.autograd.Function):
        """p = P v (adjoint False) or P^T g (True); the backward is the other direction"""

        @staticmethod
        def forward(ctx, sampler, adjoint, v):
            ctx.sampler, ctx.adjoint, ctx.like = sampler, adjoint, (v.device, v.dtype)
            return sampler._run(v, adjoint)

        @staticmethod
        def backward(ctx, g):
            return None, None, ctx.sampler._run(g, not ctx.adjoint).to(*ctx.like)

    return _ChamferFn, _SampleFn


class ChamferDistance:
    """loss = w_xy mean_i rho(dist2_xy[i]) + w_yx mean_j rho(dist2_yx[j]) between two point sets (the module's docstring has the definition).

    weights = (w_xy, w_yx), finite and >= 0; squared=True: rho(s) = s (pytorch3d's), False: rho(s) = sqrt(s), the Euclidean figure papers report.  Both are plain
    attributes read at every call; a term whose weight is 0 is not evaluated and reports 0.

    cd(x, y) takes x [N, 3] and y [M, 3] on any device and of any float dtype and returns the loss as a 0-d float32 tensor on the render device, computed on torch's
    current stream without a host synchronisation.  It is differentiable in both arguments: the forward pass produces both gradients, backward only scales them, and they
    return to the inputs' device and dtype.  cd.value_and_grad(x, y) returns (loss, dloss / dx, dloss / dy) detached.  cd.terms holds the detached [2] tensor of the two
    direction means of the last call; cd.nearest its four arrays (index_xy int32 [N], dist2_xy float32 [N], index_yx int32 [M], dist2_yx float32 [M]), None for a
    direction that is off.  Nothing is kept between calls: the sizes may change from call to call.

    search = "scan" (the default) or "grid", a plain attribute like the others: with "grid" both directions find their neighbours through a uniform grid (pointgrid.py) -
    x -> y through a grid of y, y -> x through a grid of x, each built in the call - and every result keeps the bits of the scan.  cd(x, y, y_grid=grid) and
    cd.value_and_grad(x, y, y_grid=grid) take the x -> y direction through a PointGrid of y built earlier (a fixed target: built once for a whole fit), whatever `search`
    says; the grid must be the grid of this y."""

    def __init__(self, weights=(1.0, 1.0), squared=True, search="scan"):
        # every argument is checked before a device is looked for
        self.weights, self.squared, self.search = _checked_weights(weights), bool(squared), _pg._checked_search(search, "ChamferDistance")
        self.terms = self.nearest = None

    def _checked_args(self, x, y, y_grid):
        x, y = _checked_points(x, "ChamferDistance", "x"), _checked_points(y, "ChamferDistance", "y")
        _pg._checked_search(self.search, "ChamferDistance")
        if y_grid is not None and _pg._checked_grid(y_grid, "ChamferDistance", "y_grid").points.shape[0] != y.shape[0]:
            raise ValueError("ChamferDistance: y_grid holds %d points, y has %d" % (y_grid.points.shape[0], y.shape[0]))
        return x, y

    def _eval(self, x, y, want_grad, y_grid=None):
        """-> (out [3]: the loss and the two direction means, dloss / dx [N, 3] or None, dloss / dy [M, 3] or None), on the current stream"""
        w = _checked_weights(self.weights)
        x, y = self._checked_args(x, y, y_grid)
        _single_gpu("ChamferDistance")
        import torch
        from . import cabi, _device, _stream_ptr
        device = _device()
        x, y = x.detach().to(device, torch.float32).contiguous(), y.detach().to(device, torch.float32).contiguous()
        n, m = int(x.shape[0]), int(y.shape[0])
        ptr = lambda t: None if t is None else t.data_ptr()
        with torch.cuda.device(device):
            ixy = dxy = iyx = dyx = xb = xl = yb = yl = None
            if w[0] > 0.0:
                if y_grid is not None or self.search == "grid":
                    if y_grid is not None:
                        _pg._on_render_device(y_grid, device, "ChamferDistance", "y_grid")
                    ixy, dxy, _ = _pg._grid_nearest(x, y_grid if y_grid is not None else _pg.PointGrid(y), device)
                else:
                    ixy, dxy = _nearest(x, y, device)
                if want_grad:
                    yb, yl = _inverted(ixy, m)
            if w[1] > 0.0:
                iyx, dyx = _pg._grid_nearest(y, _pg.PointGrid(x), device)[:2] if self.search == "grid" else _nearest(y, x, device)
                if want_grad:
                    xb, xl = _inverted(iyx, n)
            out = torch.empty(3, device=device, dtype=torch.float32)
            partial = torch.empty(_ceil_div(n, THREADS) + _ceil_div(m, THREADS), device=device, dtype=torch.float64)
            gx, gy = (torch.empty_like(x), torch.empty_like(y)) if want_grad else (None, None)
            cabi.check(cabi.lib().psdr_hip_chamfer_eval(x.data_ptr(), n, y.data_ptr(), m, ptr(ixy), ptr(dxy), ptr(iyx), ptr(dyx), ptr(xb), ptr(xl), ptr(yb), ptr(yl),
                                                        (_C.c_float * 2)(*w), 1 if self.squared else 0, partial.data_ptr(), out.data_ptr(), ptr(gx), ptr(gy), _stream_ptr()))
        self.terms, self.nearest = out[1:], (ixy, dxy, iyx, dyx)
        return out, gx, gy

    def __call__(self, x, y, y_grid=None):
        """the loss, a 0-d tensor"""
        x, y = self._checked_args(x, y, y_grid)
        return _fns()[0].apply(self, x, y, y_grid)

    def value_and_grad(self, x, y, y_grid=None):
        """(loss, dloss / dx, dloss / dy) without autograd, all detached: what a hand-written adjoint needs"""
        out, gx, gy = self._eval(x, y, True, y_grid)
        return out[0], gx, gy


# ---- points from a mesh's surface

SamplingCsr = _collections.namedtuple("SamplingCsr", [
    "num_vertices_in", "num_vertices_out",      # n, num_points: the names the subdivision operator's handle reads
    "row_begin", "col", "weight",               # P   [num_points x n]: three entries per row, the drawn face's vertices in the face's order, float32 barycentrics
    "t_row_begin", "t_col", "t_weight",         # P^T [n x num_points], the same float32 values, rows ascending inside a column
])


def sample_surface(v, faces, num_points, rng):
    """Draws num_points points on the triangles `faces` [f, 3] of the vertices v [n, 3]: (face int32 [num_points], bary float64 [num_points, 3]).  Host-side numpy.

    Faces are drawn in proportion to their float64 area by a stratified inversion: u_k = (k + xi_k) / num_points against the area CDF, so that face f receives within 2
    of num_points area_f / total points, in ascending face order.  A face of zero area draws nothing; a mesh whose total area is zero (or not finite) is a ValueError.
    The barycentrics are (1 - sqrt(r1), sqrt(r1) (1 - r2), sqrt(r1) r2), uniform on the triangle.  rng: a numpy.random.Generator, advanced by 3 num_points doubles."""
    v, f, k = _np.asarray(v, _np.float64), _np.asarray(faces, _np.int64), int(num_points)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    area = 0.5 * _np.sqrt((_np.cross(b - a, c - a) ** 2).sum(1))
    cdf = _np.cumsum(area)
    total = cdf[-1] if cdf.size else 0.0
    if not (_np.isfinite(total) and total > 0.0):
        raise ValueError("sample_surface: the mesh's total area is %r, nothing to draw from" % (float(total),))
    cdf = cdf / total                                            # ends at exactly 1
    xi = rng.random((k, 3))
    u = _np.minimum((_np.arange(k) + xi[:, 0]) / k, _np.nextafter(1.0, 0.0))
    face = _np.searchsorted(cdf, u, side="right")               # the first face whose CDF exceeds u: a face of zero area never is
    s = _np.sqrt(xi[:, 1])
    bary = _np.stack([1.0 - s, s * (1.0 - xi[:, 2]), s * xi[:, 2]], 1)
    return face.astype(_np.int32), bary


def sampling_csr(faces, num_vertices, face, bary):
    """The drawn points as a sparse matrix P [num_points x n] and its transpose: a SamplingCsr.  Row k holds bary[k] rounded to float32 on the vertices of faces[face[k]]"""
    f, n, k = _np.asarray(faces, _np.int64), int(num_vertices), int(len(face))
    col = f[_np.asarray(face, _np.int64)].reshape(-1)
    w = _np.asarray(bary, _np.float64).astype(_np.float32).reshape(-1)
    row = _np.repeat(_np.arange(k, dtype=_np.int64), 3)
    order = _np.argsort(col, kind="stable")                      # by column; inside a column the rows keep their ascending order
    t_begin = _np.zeros(n + 1, dtype=_np.int64)
    _np.cumsum(_np.bincount(col, minlength=n), out=t_begin[1:])
    i32 = _np.int32
    return SamplingCsr(n, k, (3 * _np.arange(k + 1, dtype=_np.int64)).astype(i32), col.astype(i32), w,
                       t_begin.astype(i32), row[order].astype(i32), _np.ascontiguousarray(w[order]))


class SurfaceSampler:
    """num_points points on the surface of a triangle mesh, as a linear operator on its vertex positions.

    mesh_or_faces: a Mesh (its face_indices and num_vertices are read) or a [f, 3] array of vertex ids with `num_vertices`; a face with a repeated id or an id out of
    range is a ValueError.  seed: of the numpy.random.Generator every resample draws from.

    resample(v) draws the points anew for the vertex positions v [num_vertices, 3] (sample_surface: area-proportional, stratified).  It is host-side numpy on a snapshot
    of v: a tensor on the GPU is copied to the host, WHICH SYNCHRONISES.  Call it once, or every k steps.  The choice (sampler.faces, sampler.bary, sampler.csr()) is
    frozen until the next resample, so that the points are linear in v.

    sampler(v) = P v returns the float32 [num_points, 3] points on the render device, on torch's current stream, differentiable in v (the backward applies P^T; gradients
    return to v's device and dtype).  The products are the subdivision operator's (psdr_hip_subdiv_apply / _apply_adj: a gather per row, no atomics, the same input gives
    the same bits).  The first call after a resample uploads the matrix (psdr_hip_subdiv_create), which synchronises the stream once.  One GPU."""

    def __init__(self, mesh_or_faces, num_vertices=None, num_points=10000, seed=0):
        if hasattr(mesh_or_faces, "face_indices") and hasattr(mesh_or_faces, "num_vertices"):
            faces = _np.asarray(mesh_or_faces.face_indices).reshape(-1, 3)
            num_vertices = int(mesh_or_faces.num_vertices) if num_vertices is None else int(num_vertices)
        else:
            faces = _np.asarray(mesh_or_faces)
            if num_vertices is None:
                raise ValueError("SurfaceSampler: num_vertices is required with a face array")
        self.num_vertices = int(num_vertices)
        self.mesh_faces = _faces_checked(faces, self.num_vertices, "SurfaceSampler")
        if self.mesh_faces.shape[0] == 0:
            raise ValueError("SurfaceSampler: the mesh has no faces")
        if int(num_points) != num_points or not 1 <= int(num_points) <= MAX_COUNT:
            raise ValueError("SurfaceSampler: num_points must be an integer in [1, 2^26], got %r" % (num_points,))
        self.num_points = int(num_points)
        self._rng = _np.random.default_rng(seed)
        self.faces = self.bary = self._csr = self._handle = None

    def resample(self, v):
        """draws the points for the positions v [num_vertices, 3] (host-side; synchronises when v is on the GPU); returns self"""
        if hasattr(v, "detach"):
            v = v.detach().cpu().double().numpy()
        v = _np.asarray(v, _np.float64)
        if v.shape != (self.num_vertices, 3):
            raise ValueError("SurfaceSampler: v must be [%d, 3], got %s" % (self.num_vertices, tuple(v.shape)))
        if not _np.isfinite(v).all():
            raise ValueError("SurfaceSampler: v holds a value that is not finite")
        self.faces, self.bary = sample_surface(v, self.mesh_faces, self.num_points, self._rng)
        self._csr = sampling_csr(self.mesh_faces, self.num_vertices, self.faces, self.bary)
        self._handle = None
        return self

    def csr(self, transpose=False):
        """(row_begin, col, weight) of P, or of P^T, as numpy arrays: what the device holds"""
        if self._csr is None:
            raise ValueError("SurfaceSampler: call resample(v) first")
        c = self._csr
        return (c.t_row_begin, c.t_col, c.t_weight) if transpose else (c.row_begin, c.col, c.weight)

    def _run(self, x, adjoint):
        import torch
        from . import cabi, _device, _stream_ptr
        from .subdiv import _Handle
        device = _device()
        x = x.detach().to(device, torch.float32).contiguous()
        with torch.cuda.device(device):
            if self._handle is None:
                self._handle = _Handle(self._csr, _stream_ptr())
            y = torch.empty((self.num_vertices if adjoint else self.num_points, 3), device=device, dtype=torch.float32)
            L = cabi.lib()
            cabi.check((L.psdr_hip_subdiv_apply_adj if adjoint else L.psdr_hip_subdiv_apply)(self._handle.ptr, x.data_ptr(), 3, y.data_ptr(), _stream_ptr()))
        return y

    def _checked(self, x, rows, name):
        import torch
        if self._csr is None:
            raise ValueError("SurfaceSampler: call resample(v) first")
        if not isinstance(x, torch.Tensor):
            x = torch.as_tensor(_np.asarray(x))
        if tuple(x.shape) != (rows, 3) or not x.is_floating_point():
            raise ValueError("SurfaceSampler: %s must be a floating-point [%d, 3] tensor, got %s %s" % (name, rows, x.dtype, tuple(x.shape)))
        _single_gpu("SurfaceSampler")
        return x

    def __call__(self, v):
        """the points P v: [num_vertices, 3] -> [num_points, 3]"""
        return _fns()[1].apply(self, False, self._checked(v, self.num_vertices, "v"))

    def transpose(self, g):
        """P^T g: [num_points, 3] -> [num_vertices, 3], what the backward of sampler(v) applies"""
        return _fns()[1].apply(self, True, self._checked(g, self.num_points, "g"))
