"""The signed distance to a mesh: for every point the generalized winding number of the mesh (the sign), the distance to the nearest face signed by it, and the gradients of that
signed distance with respect to the points and the vertices (kernels: csrc/hip/sdf.hip).

PointMeshDistance, ChamferDistance and MeshRegularizer are unsigned: none can say which side of a surface a point lies on.  With a sign a penetration penalty between two
meshes, a containment or free-space constraint, and supervision against signed distance samples can be written:

    sd = psdr.SignedDistance(mesh_b)
    penalty = torch.relu(-sd(v_a, v_b)).square().sum()          # the vertices of a that lie inside b

The definition is stated once, in include/psdr_hip.h (THE SIGNED DISTANCE).  For a point p and a face (A, B, C): a = A - p, b = B - p, c = C - p, la, lb, lc their lengths,
    Nm = a . (b x c),   Dn = ((la lb) lc + (a.b) lc) + ((b.c) la + (c.a) lb),   theta(p, f) = 0 if Nm == 0 else atan2(Nm, Dn)
the half solid angle of Van Oosterom & Strackee; the Nm == 0 branch is the principal value: a point in the face's plane, on a vertex, or a face of zero area contributes 0 and no
pair gives a NaN.  Then
    w[i] = (1 / (2 pi)) sum_f theta(p_i, f)          the generalized winding number (Jacobson et al. 2013): 1 inside, 0 outside, degrading smoothly at holes
    inside[i] = orientation w[i] > 1 / 2             orientation = +1: the faces wind counter-clockwise seen from outside; -1: the other winding
    s[i] = (inside ? -1 : +1) sqrt(D_p[i])           D_p, the face a(i) and the barycentrics exactly those of closest_points_on_mesh
A sign from normals or pseudonormals is wrong near the boundary edges of an open mesh (bunny_low.obj has 42); the winding number is not.

The gradient is that of s alone, with indices, barycentrics and the sign held constant: ds_i / dp_i = r_i / s_i and ds_i / dv[faces[a(i)][c]] = -bary_ic r_i / s_i with
r_i = p_i - q_i, both 0 where D_p[i] = 0.  w and inside carry no gradient: for a closed mesh the winding number is piecewise constant, and its analytic vertex gradient cancels
to 1e-17 in float64 - it is the sign, not a differentiable quantity.  The backward pass gathers in fixed orders through an inverted index built on the device: no float atomics,
the same input gives the same bits.

The winding scan splits the faces into the slices of launch_plan_pm(N, F) and adds slice sums in ascending order, so the last bits of w depend on that plan - a pure function of
(N, F).  Nothing of size N x F exists and nothing synchronises with the host.  One GPU only: under an initialised torch.distributed group of more than one rank the calls raise."""
import collections as _collections
import functools as _functools

import numpy as _np

from ._opcommon import _checked_points, _inverted, _single_gpu
from .pointmesh import _checked_faces, _checked_vertices, _device_topology, _function_arguments, _on_device, _scan, launch_plan_pm

SignedDistanceResult = _collections.namedtuple("SignedDistanceResult", ["sdf", "winding", "face", "bary", "dist2"])
Nearest = _collections.namedtuple("Nearest", ["face", "bary", "dist2"])


def _checked_orientation(orientation, what):
    if isinstance(orientation, bool) or not isinstance(orientation, (int, _np.integer)) or int(orientation) not in (1, -1):
        raise ValueError("%s: orientation must be +1 (the faces wind counter-clockwise seen from outside) or -1, got %r" % (what, orientation))
    return int(orientation)


def _winding(points, v, faces, dist2, orientation, device):
    """points, v: float32 contiguous on `device`, faces int32 [F, 3] there, dist2 float32 [N] or None -> (w float32 [N], s float32 [N] or None), on the current stream"""
    import torch
    from . import cabi, _stream_ptr
    N, n, F = int(points.shape[0]), int(v.shape[0]), int(faces.shape[0])
    records = torch.empty((F, 12), device=device, dtype=torch.float32)
    partial = torch.empty((launch_plan_pm(N, F).slices, N), device=device, dtype=torch.float32)
    w = torch.empty(N, device=device, dtype=torch.float32)
    s = None if dist2 is None else torch.empty(N, device=device, dtype=torch.float32)
    cabi.check(cabi.lib().psdr_hip_sdf_winding(points.data_ptr(), N, v.data_ptr(), n, faces.data_ptr(), F, records.data_ptr(), partial.data_ptr(),
                                               None if dist2 is None else dist2.data_ptr(), orientation, w.data_ptr(), None if s is None else s.data_ptr(), _stream_ptr()))
    return w, s


def winding_number(points, v, faces):
    """The generalized winding number of the mesh (v, faces) at every point: float32 [N] on the render device, detached, computed on torch's current stream without a host
    synchronisation.  1 inside and 0 outside a closed mesh whose faces wind counter-clockwise seen from outside (-1 inside for the other winding), 2 where two closed
    components overlap, and in between near the holes of an open mesh.  It carries no gradient (the module docstring says why).

    The argument rules are closest_points_on_mesh's: points [N, 3] and v [n, 3] on any device and of any float dtype; faces on the host are checked like a mesh's (a repeated
    or out-of-range id is a ValueError) and uploaded at every call, which waits for the copy; an int32 tensor that already lies on a GPU is used as it is - the kernels clamp
    every id into range - and then nothing synchronises."""
    import torch
    what = "winding_number"
    device, p, vd, fd = _on_device(*_function_arguments(points, v, faces, what), what)
    with torch.cuda.device(device):
        return _winding(p, vd, fd, None, 1, device)[0]


def signed_distance(points, v, faces, orientation=1):
    """SignedDistanceResult(sdf, winding, face, bary, dist2), all detached on the render device and torch's current stream: sdf float32 [N] = -sqrt(dist2) where
    orientation winding > 1 / 2, else +sqrt(dist2); face int32 [N], bary float32 [N, 3] and dist2 float32 [N] are closest_points_on_mesh's, bit for bit.  The argument rules
    are winding_number's; orientation is +1 (the faces wind counter-clockwise seen from outside) or -1."""
    import torch
    what = "signed_distance"
    args = _function_arguments(points, v, faces, what)
    orientation = _checked_orientation(orientation, what)
    device, p, vd, fd = _on_device(*args, what)
    with torch.cuda.device(device):
        face, bary, dist2 = _scan(p, vd, fd, 0, device)
        w, s = _winding(p, vd, fd, dist2, orientation, device)
    return SignedDistanceResult(s, w, face, bary, dist2)


@_functools.lru_cache(maxsize=None)
def _fn():
    import torch

    class _SignedDistanceFn(torch.autograd.Function):
        """sd(points, v): the incoming gradient is a vector, so the vector-Jacobian product runs in the backward pass"""

        @staticmethod
        def forward(ctx, sd, points, v):
            device, p, vd, s, face, bary = sd._forward(points, v)
            ctx.save_for_backward(p, vd, s, face, bary)
            ctx.sd, ctx.device = sd, device
            ctx.like = ((points.device, points.dtype), (v.device, v.dtype))
            return s

        @staticmethod
        def backward(ctx, g):
            p, vd, s, face, bary = ctx.saved_tensors
            gp, gv = ctx.sd._grad(ctx.device, p, vd, s, face, bary, g.detach().to(ctx.device, torch.float32).contiguous())
            return None, gp.to(*ctx.like[0]) if ctx.needs_input_grad[1] else None, gv.to(*ctx.like[1]) if ctx.needs_input_grad[2] else None

    return _SignedDistanceFn


class SignedDistance:
    """s[i] = -+ the distance from points[i] to the nearest face of one mesh topology, negative where the generalized winding number says inside (include/psdr_hip.h has the
    definition).

    mesh_or_faces: a Mesh (its face_indices and num_vertices are read) or a [F, 3] array of vertex ids with `num_vertices`; a face with a repeated id or an id out of range
    is a ValueError.  orientation: +1 where the faces wind counter-clockwise seen from outside, -1 for the other winding; a plain attribute read at every call, anything else
    is a ValueError.

    sd(points, v) takes points [N, 3] and v [num_vertices, 3] on any device and of any float dtype and returns s as a float32 [N] tensor on the render device, computed on
    torch's current stream without a host synchronisation.  It is differentiable in both arguments with indices, barycentrics and sign held constant; the backward pass runs
    three launches for the incoming gradient vector and the gradients return to the inputs' device and dtype.  sd.vjp(points, v, g) returns (s, g . ds / dpoints [N, 3],
    g . ds / dv [num_vertices, 3]) detached, the same bits.  sd.winding holds the detached winding numbers float32 [N] of the last call and sd.nearest its (face int32 [N],
    bary [N, 3], dist2 [N]), closest_points_on_mesh's bit for bit.  Neither the winding number nor the sign carries a gradient (the module docstring says why).  The faces and
    the vertex-to-corner index go to the device at the first call; nothing else is kept between calls: N may change from call to call."""

    def __init__(self, mesh_or_faces, num_vertices=None, orientation=1):
        # every argument is checked before a device is looked for
        self.faces, self.num_vertices = _checked_faces(mesh_or_faces, num_vertices, "SignedDistance")
        self.orientation = _checked_orientation(orientation, "SignedDistance")
        self.winding = self.nearest = None
        self._topology = None

    def _checked(self, points, v):
        return _checked_points(points, "SignedDistance", "points"), _checked_vertices(v, self.num_vertices, "SignedDistance"), _checked_orientation(self.orientation, "SignedDistance")

    def _forward(self, points, v):
        """-> (device, points, v float32 on it, s [N], face [N], bary [N, 3]), on the current stream"""
        points, v, orientation = self._checked(points, v)
        _single_gpu("SignedDistance")
        import torch
        from . import _device
        device = _device()
        p, vd = points.detach().to(device, torch.float32).contiguous(), v.detach().to(device, torch.float32).contiguous()
        with torch.cuda.device(device):
            faces = _device_topology(self, device)[0]
            face, bary, dist2 = _scan(p, vd, faces, 0, device)
            w, s = _winding(p, vd, faces, dist2, orientation, device)
        self.winding, self.nearest = w, Nearest(face, bary, dist2)
        return device, p, vd, s, face, bary

    def _grad(self, device, p, vd, s, face, bary, g):
        """the vector-Jacobian product for g float32 [N] on `device` -> (gp [N, 3], gv [n, 3]), on the current stream"""
        import torch
        from . import cabi, _stream_ptr
        N, n, F = int(p.shape[0]), self.num_vertices, int(self.faces.shape[0])
        with torch.cuda.device(device):
            faces, vc_begin, vc_corner = _device_topology(self, device)
            f_begin, f_list = _inverted(face, F)
            gp, gv = torch.empty_like(p), torch.empty_like(vd)
            corners = torch.empty((F, 9), device=device, dtype=torch.float32)
            cabi.check(cabi.lib().psdr_hip_sdf_grad(p.data_ptr(), N, vd.data_ptr(), n, faces.data_ptr(), F, face.data_ptr(), bary.data_ptr(), s.data_ptr(), g.data_ptr(),
                                                    f_begin.data_ptr(), f_list.data_ptr(), vc_begin.data_ptr(), vc_corner.data_ptr(), corners.data_ptr(),
                                                    gp.data_ptr(), gv.data_ptr(), _stream_ptr()))
        return gp, gv

    def __call__(self, points, v):
        """the signed distances, a float32 [N] tensor"""
        points, v, _orientation = self._checked(points, v)
        return _fn().apply(self, points, v)

    def vjp(self, points, v, g):
        """(s, g . ds / dpoints, g . ds / dv) without autograd, all detached: what a hand-written adjoint needs.  g: [N], any device, any float dtype"""
        import torch
        points, v, _orientation = self._checked(points, v)
        if not isinstance(g, torch.Tensor):
            g = torch.as_tensor(_np.asarray(g))
        if tuple(g.shape) != (int(points.shape[0]),) or not g.is_floating_point():
            raise ValueError("SignedDistance: g must be a floating-point [%d] tensor, got %s %s" % (int(points.shape[0]), g.dtype, tuple(g.shape)))
        device, p, vd, s, face, bary = self._forward(points, v)
        gp, gv = self._grad(device, p, vd, s, face, bary, g.detach().to(device, torch.float32).contiguous())
        return s, gp, gv
