"""The point-to-mesh distance: for every point the nearest face of a triangle mesh, for every face the nearest point, value and the gradients with respect to the points
and the vertices (kernels: csrc/hip/pointmesh.hip).

ChamferDistance between sampled points and a cloud measures the surface through a frozen sample: it synchronises on every resample and its error floor is the sample
spacing.  This measures the distance to the closed triangles themselves (pytorch3d's point_mesh_face_distance is the one users know) - a point that lies on a face is at
distance 0:

    pm = psdr.PointMeshDistance(mesh, weights=(1.0, 1.0))
    loss = ms(img, target) + reg(v) + w * pm(scan_points, v)

The definition is stated once, in include/psdr_hip.h (THE POINT-TO-MESH DISTANCE): the pair function cp(p; a, b, c) - Ericson's seven-region cascade for the closest point of
a closed triangle, as barycentrics, every operation one float32 rounding - and dist2 = |(p - a) - (s ab + t ac)|^2, the difference form; then
    D_p[i] = min_f dist2(p_i, f), a(i) the lowest such f;   D_f[f] = min_i dist2(p_i, f), b(f) the lowest such i
    loss   = w_pf (1 / N) sum_i rho(D_p[i]) + w_fp (1 / F) sum_f rho(D_f[f])      rho(s) = s (squared=True) or sqrt(s), with derivative 0 at s = 0; a term of weight 0
                                                                                    is not evaluated
    gradient  indices and barycentrics are constants - for the squared distance the exact derivative, by the envelope theorem.  Every point and every face corner adds
              its own pair and then, through inverted indices built on the device at every call (a stable sort), the pairs that chose it in ascending order; a vertex adds
              the records of its corners in the order of the mesh's vertex-to-corner index (from the host, once per object).  No float atomics: the same input gives
              the same bits.
Written in torch ops this is an N x F broadcast of the cascade, some thirty [N, F] temporaries, and an index_add_ backward on float atomics.  Here two scans keep the
queries in registers and stream the candidates through LDS; nothing of size N x F exists and nothing synchronises with the host.

A face of zero area or with an edge of zero length gives a finite point of the triangle, never a NaN; it is the closest point except where a face's first two vertices
coincide in position, where the cascade returns that vertex.

launch_plan_pm(n_queries, n_candidates) is the scans' split into query blocks x candidate slices, which psdr_hip_pointmesh_plan states in C; the result does not
depend on it.  One GPU only: under an initialised torch.distributed group of more than one rank the calls raise."""
import collections as _collections
import ctypes as _C
import functools as _functools
import math as _math

import numpy as _np

from ._opcommon import MAX_COUNT, NARROW_MAX, TARGET_GROUPS, SCAN_THREADS as THREADS, _ceil_div, _checked_points, _faces_checked, _inverted, _single_gpu, _vertex_index, slice_plan  # noqa: F401

TILE = 256                   # candidates per LDS tile
WIDE_QUERIES = 2             # queries per lane for n_queries > NARROW_MAX, else 1

LaunchPlan = _collections.namedtuple("LaunchPlan", ["tile", "queries_per_lane", "slices", "slice_len"])
Nearest = _collections.namedtuple("Nearest", ["face_of_point", "bary_p", "dist2_p", "point_of_face", "bary_f", "dist2_f"])


def launch_plan_pm(n_queries, n_candidates):
    """How a scan of n_queries over n_candidates is split: LaunchPlan(tile, queries_per_lane, slices, slice_len), a pure function (csrc/hip/pointmesh.hip: plan_of).

    A workgroup holds 256 queries_per_lane queries; slice s holds the candidates [s slice_len, min(n_candidates, (s + 1) slice_len)); the grid is query blocks x slices.
    The same split serves both scans: points against faces and faces against points."""
    n, m = int(n_queries), int(n_candidates)
    return LaunchPlan(*slice_plan(n, m, TILE, WIDE_QUERIES, "launch_plan_pm: n_queries = %d, n_candidates = %d, both must lie in [1, 2^26]" % (n, m)))


def _checked_weights(weights):
    try:
        w = tuple(float(x) for x in weights)
    except (TypeError, ValueError):
        raise ValueError("PointMeshDistance: weights must be two numbers (point -> face, face -> point), got %r" % (weights,)) from None
    if len(w) != 2 or not all(_math.isfinite(x) and x >= 0.0 for x in w):
        raise ValueError("PointMeshDistance: weights must be two finite numbers >= 0 (point -> face, face -> point), got %r" % (weights,))
    return w


def _checked_faces(mesh_or_faces, num_vertices, what):
    """-> (faces int64 [F, 3] with F >= 1, num_vertices)"""
    if hasattr(mesh_or_faces, "face_indices") and hasattr(mesh_or_faces, "num_vertices"):
        faces = _np.asarray(mesh_or_faces.face_indices).reshape(-1, 3)
        num_vertices = int(mesh_or_faces.num_vertices) if num_vertices is None else int(num_vertices)
    else:
        faces = _np.asarray(mesh_or_faces)
        if num_vertices is None:
            raise ValueError("%s: num_vertices is required with a face array" % what)
    f = _faces_checked(faces, int(num_vertices), what)
    if f.shape[0] == 0:
        raise ValueError("%s: the mesh has no faces" % what)
    if f.shape[0] > MAX_COUNT:
        raise ValueError("%s: %d faces, at most 2^26" % (what, f.shape[0]))
    return f, int(num_vertices)


def _checked_vertices(v, n, what):
    import torch
    if not isinstance(v, torch.Tensor):
        v = torch.as_tensor(_np.asarray(v))
    if tuple(v.shape) != (n, 3) or not v.is_floating_point():
        raise ValueError("%s: v must be a floating-point [%d, 3] tensor, got %s %s" % (what, n, v.dtype, tuple(v.shape)))
    return v


def _scan(points, v, faces, direction, device):
    """points, v: float32 contiguous on `device`, faces int32 [F, 3] there -> (index int32, bary float32 [., 3], dist2 float32) per query, on the current stream"""
    import torch
    from . import cabi, _stream_ptr
    N, n, F = int(points.shape[0]), int(v.shape[0]), int(faces.shape[0])
    count = F if direction else N
    keys = torch.empty(count, device=device, dtype=torch.int64)
    index = torch.empty(count, device=device, dtype=torch.int32)
    bary = torch.empty((count, 3), device=device, dtype=torch.float32)
    dist2 = torch.empty(count, device=device, dtype=torch.float32)
    records = None if direction else torch.empty((F, 16), device=device, dtype=torch.float32)
    cabi.check(cabi.lib().psdr_hip_pointmesh_nearest(points.data_ptr(), N, v.data_ptr(), n, faces.data_ptr(), F, direction, None if direction else records.data_ptr(),
                                                     keys.data_ptr(), index.data_ptr(), bary.data_ptr(), dist2.data_ptr(), _stream_ptr()))
    return index, bary, dist2


def _function_arguments(points, v, faces, what):
    """the argument rules of closest_points_on_mesh (and of sdf.py's functions), before a device is looked for -> (points, v, faces on a GPU or None, host faces int64 or
    None)"""
    import torch
    points = _checked_points(points, what, "points")
    if not hasattr(v, "shape") or len(v.shape) != 2 or int(v.shape[0]) < 1:
        raise ValueError("%s: v must be [n, 3] with n >= 1" % what)
    n = int(v.shape[0])
    v = _checked_vertices(v, n, what)
    if isinstance(faces, torch.Tensor) and faces.is_cuda:
        if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3 or not 1 <= faces.shape[0] <= MAX_COUNT:
            raise ValueError("%s: faces on the GPU must be an int32 [F, 3] tensor with 1 <= F <= 2^26, got %s %s" % (what, faces.dtype, tuple(faces.shape)))
        if n > MAX_COUNT:
            raise ValueError("%s: %d vertices, at most 2^26" % (what, n))
        return points, v, faces, None
    f, n = _checked_faces(faces.detach().numpy() if isinstance(faces, torch.Tensor) else faces, n, what)
    return points, v, None, f


def _on_device(points, v, faces_gpu, faces_host, what):
    """-> (device, points, v, faces) float32 / int32 contiguous on the render device"""
    import torch
    _single_gpu(what)
    from . import _device
    device = _device()
    with torch.cuda.device(device):
        fd = faces_gpu.to(device).contiguous() if faces_host is None else torch.from_numpy(_np.ascontiguousarray(faces_host, _np.int32)).to(device)
        return device, points.detach().to(device, torch.float32).contiguous(), v.detach().to(device, torch.float32).contiguous(), fd


def _device_topology(obj, device):
    """(faces int32 [F, 3], vc_begin int32 [n + 1], vc_corner int32 [3 F]) of obj.faces / obj.num_vertices on `device`: uploaded once per object, kept in obj._topology (the
    copies are ordered on the current stream)"""
    import torch
    if obj._topology is None or obj._topology[0] != device:
        begin, elem, role = _vertex_index(obj.faces, obj.num_vertices)
        corner = (3 * elem.astype(_np.int64) + role).astype(_np.int32)
        up = lambda a: torch.from_numpy(_np.ascontiguousarray(a, _np.int32)).to(device)
        obj._topology = (device, up(obj.faces), up(begin), up(corner))
    return obj._topology[1:]


def closest_points_on_mesh(points, v, faces):
    """For every point the lowest index of its nearest face, the barycentrics of the closest point on it and the squared distance: (face int32 [N], bary float32 [N, 3],
    dist2 float32 [N]) on the render device, detached, computed on torch's current stream without a host synchronisation.  points [N, 3] and v [n, 3] on any device and of
    any float dtype, faces [F, 3] integer ids in [0, n); the closest point is bary . v[faces[face]].

    faces on the host (an array, a list, a CPU tensor) are checked like a mesh's (a repeated or out-of-range id is a ValueError) and uploaded at every call, which waits
    for the copy; an int32 tensor that already lies on a GPU is used as it is - the kernels clamp every id into range - and then nothing synchronises."""
    import torch
    what = "closest_points_on_mesh"
    device, p, vd, fd = _on_device(*_function_arguments(points, v, faces, what), what)
    with torch.cuda.device(device):
        return _scan(p, vd, fd, 0, device)


@_functools.lru_cache(maxsize=None)
def _fn():
    import torch

    class _PointMeshFn(torch.autograd.Function):
        """pm(points, v): the forward also produces both gradients, the backward scales them by the incoming scalar"""

        @staticmethod
        def forward(ctx, pm, points, v):
            out, gp, gv = pm._eval(points, v, True)
            ctx.save_for_backward(gp, gv)
            ctx.like = ((points.device, points.dtype), (v.device, v.dtype))
            return out[0]

        @staticmethod
        def backward(ctx, g):
            gp, gv = ctx.saved_tensors
            return None, (g * gp).to(*ctx.like[0]) if ctx.needs_input_grad[1] else None, (g * gv).to(*ctx.like[1]) if ctx.needs_input_grad[2] else None

    return _PointMeshFn


class PointMeshDistance:
    """loss = w_pf mean_i rho(D_p[i]) + w_fp mean_f rho(D_f[f]) between a point set and the faces of one mesh topology (include/psdr_hip.h has the definition).

    mesh_or_faces: a Mesh (its face_indices and num_vertices are read) or a [F, 3] array of vertex ids with `num_vertices`; a face with a repeated id or an id out of
    range is a ValueError.  weights = (w_pf, w_fp): points to their nearest faces, faces to their nearest points, finite and >= 0; squared=True: rho(s) = s
    (pytorch3d's), False: rho(s) = sqrt(s).  Both are plain attributes read at every call; a term whose weight is 0 is not evaluated and reports 0.

    pm(points, v) takes points [N, 3] and v [num_vertices, 3] on any device and of any float dtype and returns the loss as a 0-d float32 tensor on the render device,
    computed on torch's current stream without a host synchronisation.  It is differentiable in both arguments: the forward pass produces both gradients, backward only
    scales them, and they return to the inputs' device and dtype.  pm.value_and_grad(points, v) returns (loss, dloss / dpoints, dloss / dv) detached.  pm.terms holds the
    detached [2] tensor of the two direction means of the last call; pm.nearest its six arrays (face_of_point int32 [N], bary_p [N, 3], dist2_p [N], point_of_face int32
    [F], bary_f [F, 3], dist2_f [F]), None for a direction that is off.  The faces and the vertex-to-corner index go to the device at the first call; nothing else is
    kept between calls: N may change from call to call."""

    def __init__(self, mesh_or_faces, num_vertices=None, weights=(1.0, 1.0), squared=True):
        # every argument is checked before a device is looked for
        self.faces, self.num_vertices = _checked_faces(mesh_or_faces, num_vertices, "PointMeshDistance")
        self.weights, self.squared = _checked_weights(weights), bool(squared)
        self.terms = self.nearest = None
        self._topology = None

    def _eval(self, points, v, want_grad):
        """-> (out [3]: the loss and the two direction means, dloss / dpoints [N, 3] or None, dloss / dv [n, 3] or None), on the current stream"""
        w = _checked_weights(self.weights)
        points, v = _checked_points(points, "PointMeshDistance", "points"), _checked_vertices(v, self.num_vertices, "PointMeshDistance")
        _single_gpu("PointMeshDistance")
        import torch
        from . import cabi, _device, _stream_ptr
        device = _device()
        points, v = points.detach().to(device, torch.float32).contiguous(), v.detach().to(device, torch.float32).contiguous()
        N, n, F = int(points.shape[0]), self.num_vertices, int(self.faces.shape[0])
        ptr = lambda t: None if t is None else t.data_ptr()
        with torch.cuda.device(device):
            faces, vc_begin, vc_corner = _device_topology(self, device)
            fop = bp = dp = pof = bf = df = pb = pl = fb = fl = None
            if w[0] > 0.0:
                fop, bp, dp = _scan(points, v, faces, 0, device)
                if want_grad:
                    fb, fl = _inverted(fop, F)
            if w[1] > 0.0:
                pof, bf, df = _scan(points, v, faces, 1, device)
                if want_grad:
                    pb, pl = _inverted(pof, N)
            out = torch.empty(3, device=device, dtype=torch.float32)
            partial = torch.empty(_ceil_div(N, THREADS) + _ceil_div(F, THREADS), device=device, dtype=torch.float64)
            gp = gv = corners = None
            if want_grad:
                gp, gv = torch.empty_like(points), torch.empty_like(v)
                corners = torch.empty((F, 9), device=device, dtype=torch.float32)
            cabi.check(cabi.lib().psdr_hip_pointmesh_eval(points.data_ptr(), N, v.data_ptr(), n, faces.data_ptr(), F, ptr(fop), ptr(bp), ptr(dp), ptr(pof), ptr(bf), ptr(df),
                                                          ptr(pb), ptr(pl), ptr(fb), ptr(fl), vc_begin.data_ptr(), vc_corner.data_ptr(), (_C.c_float * 2)(*w),
                                                          1 if self.squared else 0, partial.data_ptr(), ptr(corners), out.data_ptr(), ptr(gp), ptr(gv), _stream_ptr()))
        self.terms, self.nearest = out[1:], Nearest(fop, bp, dp, pof, bf, df)
        return out, gp, gv

    def __call__(self, points, v):
        """the loss, a 0-d tensor"""
        return _fn().apply(self, _checked_points(points, "PointMeshDistance", "points"), _checked_vertices(v, self.num_vertices, "PointMeshDistance"))

    def value_and_grad(self, points, v):
        """(loss, dloss / dpoints, dloss / dv) without autograd, all detached: what a hand-written adjoint needs"""
        out, gp, gv = self._eval(points, v, True)
        return out[0], gp, gv
