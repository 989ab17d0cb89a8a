"""The mesh regularisers: uniform Laplacian smoothing, normal consistency and edge length of a triangle mesh, value and vertex gradient in one fused pass (DESIGN.md
section 7j; kernels: csrc/hip/meshreg.hip).

An image loss says nothing about back faces, occluded parts and the inside of flat regions; every pipeline that moves vertices adds a term that depends on the mesh alone
(pytorch3d's mesh_laplacian_smoothing, mesh_normal_consistency and mesh_edge_loss are the ones users know):

    ms = psdr.MultiScaleLoss(sc.opts.width, sc.opts.height)
    reg = psdr.MeshRegularizer(mesh, weights=(1.0, 0.1, 0.0))
    loss = ms(img, target) + reg(pre.from_differential(u))              # or reg(sub.refine(c))

The definition (include/psdr_hip.h states it in full).  V [n, 3]; E the distinct undirected edges (a < b) of the faces, sorted; N(i), deg_i from laplacian_csr; a hinge
(a, b, c, d) is an edge with exactly two faces, c opposite it in the first (lower face index), d in the second; n1 = (b - a) x (c - a), n2 = (d - a) x (b - a), u = n / |n|.
    laplacian = (1 / n_L) sum_i |v_i - (1 / deg_i) sum_{j in N(i)} v_j|^2        n_L = the vertices a face uses
    normal    = (1 / h) sum_hinges 1/2 |u1 - u2|^2                               0 on a flat hinge, 2 on one folded back; a hinge with a face of zero area adds nothing
    edge      = (1 / e) sum_edges (|v_a - v_b| - target_length)^2                at target_length > 0 an edge of zero length adds target_length^2 and no gradient
    loss      = w_lap laplacian + w_nor normal + w_edge edge                     a term of weight 0 is not evaluated
Written in torch ops (index_select, cross, index_add_) these are some forty launches and a backward that scatters with float atomics, whose bits change from run to run.
Here every element stores its contributions, every vertex adds its own in a fixed order: three launches, no atomics, the same input gives the same bits.

The topology (mesh_topology) is numpy and runs once per mesh on the host, usable without the native library.  There is no vertex welding.  One GPU only: under an
initialised torch.distributed group of more than one rank the calls raise."""
import collections as _collections
import ctypes as _C
import functools as _functools
import math as _math

import numpy as _np

from ._opcommon import MAX_COUNT, _faces_checked, _single_gpu, _vertex_index

MeshTopology = _collections.namedtuple("MeshTopology", [
    "edges",                    # int32 [e, 2]: the distinct undirected edges (a < b), ascending
    "hinges",                   # int32 [h, 4]: (a, b, c, d) of the edges with exactly two faces, in edge order
    "num_boundary_edges", "num_nonmanifold_edges",      # edges with one face / with three or more
    "edge_begin", "edge_elem", "edge_role",             # per vertex the (edge, role) pairs that name it, ascending: int32 [n + 1], [2 e], [2 e]; role 0, 1 = a, b
    "hinge_begin", "hinge_elem", "hinge_role",          # the same over the hinges: int32 [n + 1], [4 h], [4 h]; role 0 .. 3 = a, b, c, d
])



def mesh_topology(faces, num_vertices):
    """The edges, hinges and inverted indices of a triangle list: a MeshTopology of numpy arrays.  Host-side, no GPU, once per mesh.

    faces [f, 3] vertex ids in [0, n), n = num_vertices, f >= 0; a face with a repeated id or an id out of range is a ValueError.  No welding: a seam an OBJ file lists
    twice is a boundary here.

    edges: the distinct undirected vertex pairs (a < b), ascending.  hinges: the edges with exactly two incident faces (a duplicate face counts twice), in edge order,
    as (a, b, c, d) with c the third vertex of the incident face of lower index and d that of the other; two copies of one face give c == d.  Boundary edges (one face)
    and non-manifold edges (three or more) form no hinge and are counted.  The inverted indices list per vertex every (element, role) that names it, each exactly once,
    in ascending order - what the device's per-vertex gather walks."""
    n = int(num_vertices)
    f = _faces_checked(faces, n, "mesh_topology")
    F = f.shape[0]
    # the three half-edges of every face: block 0 is (a, b), block 1 (b, c), block 2 (c, a); `opp` the face's third vertex
    ha = _np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    hb = _np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    opp = _np.concatenate([f[:, 2], f[:, 0], f[:, 1]])
    face = _np.concatenate([_np.arange(F, dtype=_np.int64)] * 3)
    key, edge_of, m = _np.unique(_np.minimum(ha, hb) * n + _np.maximum(ha, hb), return_inverse=True, return_counts=True)
    edge_of = edge_of.reshape(-1)
    E = int(key.size)
    if E > MAX_COUNT:
        raise ValueError("mesh_topology: %d edges, at most 2^26" % E)
    edges = _np.stack([key // n, key % n], 1).reshape(E, 2)
    by_edge = _np.lexsort((face, edge_of))                         # the half-edges grouped by edge, in face order inside a group
    first = _np.cumsum(m) - m
    two = m == 2
    c, d = opp[by_edge[first[two]]], opp[by_edge[first[two] + 1]]
    hinges = _np.concatenate([edges[two], _np.stack([c, d], 1).reshape(-1, 2)], 1).reshape(-1, 4)
    eb, ee, er = _vertex_index(edges, n)
    hb_, he, hr = _vertex_index(hinges, n)
    i32 = _np.int32
    return MeshTopology(_np.ascontiguousarray(edges.astype(i32)), _np.ascontiguousarray(hinges.astype(i32)), int((m == 1).sum()), int((m >= 3).sum()),
                        eb, ee, er, hb_, he, hr)


def _checked_weights(weights):
    try:
        w = tuple(float(x) for x in weights)
    except (TypeError, ValueError):
        raise ValueError("MeshRegularizer: weights must be three numbers (laplacian, normal, edge), got %r" % (weights,)) from None
    if len(w) != 3 or not all(_math.isfinite(x) and x >= 0.0 for x in w):
        raise ValueError("MeshRegularizer: weights must be three finite numbers >= 0 (laplacian, normal, edge), got %r" % (weights,))
    return w


def _checked_length(target_length):
    try:
        t = float(target_length)
    except (TypeError, ValueError):
        raise ValueError("MeshRegularizer: target_length must be a number, got %r" % (target_length,)) from None
    if not (_math.isfinite(t) and t >= 0.0):
        raise ValueError("MeshRegularizer: target_length = %r, must be finite and >= 0" % (target_length,))
    return t


class _Handle:
    """owner of a psdr_hip_meshreg"""

    def __init__(self, n, topo, row_begin, col, stream):
        from . import cabi
        self.ptr, self._cabi = _C.c_void_p(), cabi
        arrays = [_np.ascontiguousarray(a, _np.int32) for a in (topo.edges, topo.hinges, row_begin, col, topo.edge_begin, topo.edge_elem, topo.edge_role,
                                                               topo.hinge_begin, topo.hinge_elem, topo.hinge_role)]
        cabi.check(cabi.lib().psdr_hip_meshreg_create(n, topo.edges.shape[0], topo.hinges.shape[0], *[a.ctypes.data if a.size else None for a in arrays],
                                                      _C.byref(self.ptr), stream))

    def __del__(self):
        if getattr(self, "ptr", None) and self._cabi is not None:
            self._cabi.lib().psdr_hip_meshreg_destroy(self.ptr)
            self.ptr = None


@_functools.lru_cache(maxsize=None)
def _fn():
    import torch

    class _MeshRegFn(torch.autograd.Function):
        """reg(v): the forward also produces dloss / dv, the backward scales it by the incoming scalar"""

        @staticmethod
        def forward(ctx, reg, v):
            out, grad = reg._eval(v, True)
            ctx.save_for_backward(grad)
            ctx.like = (v.device, v.dtype)
            reg.terms = out[1:]
            return out[0]

        @staticmethod
        def backward(ctx, g):
            grad, = ctx.saved_tensors
            return None, (g * grad).to(*ctx.like)

    return _MeshRegFn


class MeshRegularizer:
    """loss = w_lap laplacian + w_nor normal + w_edge edge of one mesh topology (the module's docstring has the definition).

    mesh_or_faces: a Mesh (its face_indices and num_vertices are read) or a [f, 3] array of vertex ids with `num_vertices`; a face with a repeated id or an id out of
    range is a ValueError.  weights = (w_lap, w_nor, w_edge), finite and >= 0; target_length >= 0.  Both are plain attributes read at every call, so a schedule can
    change them; a term whose weight is 0 is not evaluated and reports 0.

    reg(v) takes a [num_vertices, 3] tensor on any device and of any float dtype and returns the loss as a 0-d float32 tensor on the render device, computed on torch's
    current stream without a host synchronisation.  It is differentiable in v: the forward pass produces the gradient as well, backward only scales it, and the gradient
    returns to v's device and dtype.  reg.value_and_grad(v) returns (loss, dloss / dv) detached; reg.terms holds the detached [3] tensor (laplacian, normal, edge) of the
    last call.  reg.topology is the MeshTopology, reg.row_begin / reg.col the Laplacian pattern.

    The handle owns work frames: calls on one MeshRegularizer must follow each other on one stream."""

    def __init__(self, mesh_or_faces, num_vertices=None, weights=(1.0, 1.0, 1.0), target_length=0.0):
        if hasattr(mesh_or_faces, "face_indices") and hasattr(mesh_or_faces, "num_vertices"):
            faces = _np.asarray(mesh_or_faces.face_indices).reshape(-1, 3)
            num_vertices = int(mesh_or_faces.num_vertices) if num_vertices is None else int(num_vertices)
        else:
            faces = _np.asarray(mesh_or_faces)
            if num_vertices is None:
                raise ValueError("MeshRegularizer: num_vertices is required with a face array")
        # every argument is checked before a device is looked for
        self.weights, self.target_length = _checked_weights(weights), _checked_length(target_length)
        self.num_vertices = int(num_vertices)
        try:
            self.topology = mesh_topology(faces, self.num_vertices)
        except ValueError as e:
            raise ValueError("MeshRegularizer: " + str(e)) from None
        from .precond import laplacian_csr
        self.row_begin, self.col = laplacian_csr(_faces_checked(faces, self.num_vertices, "MeshRegularizer"), self.num_vertices)
        self.terms = None
        _single_gpu("MeshRegularizer")
        from . import _device, _stream_ptr
        import torch
        self._device = _device()
        with torch.cuda.device(self._device):
            self._handle = _Handle(self.num_vertices, self.topology, self.row_begin, self.col, _stream_ptr())

    def _eval(self, v, want_grad):
        """-> (out [4]: the loss and the three terms, dloss / dv [n, 3] or None), on the current stream"""
        import torch
        from . import cabi, _stream_ptr
        _single_gpu("MeshRegularizer")
        w, t = _checked_weights(self.weights), _checked_length(self.target_length)
        if not isinstance(v, torch.Tensor) or tuple(v.shape) != (self.num_vertices, 3) or not v.is_floating_point():
            raise ValueError("MeshRegularizer: v must be a floating-point [%d, 3] tensor, got %s" % (self.num_vertices, tuple(v.shape) if hasattr(v, "shape") else type(v)))
        v = v.detach().to(self._device, torch.float32).contiguous()
        with torch.cuda.device(self._device):
            out = torch.empty(4, device=self._device, dtype=torch.float32)
            grad = torch.empty_like(v) if want_grad else None
            cabi.check(cabi.lib().psdr_hip_meshreg_eval(self._handle.ptr, v.data_ptr(), (_C.c_float * 3)(*w), t, out.data_ptr(), grad.data_ptr() if want_grad else None,
                                                        _stream_ptr()))
        return out, grad

    @staticmethod
    def _tensor(x):
        import torch
        return x if isinstance(x, torch.Tensor) else torch.as_tensor(_np.asarray(x))

    def __call__(self, v):
        """the loss, a 0-d tensor"""
        return _fn().apply(self, self._tensor(v))

    def value_and_grad(self, v):
        """(loss, dloss / dv) without autograd, both detached: what a hand-written adjoint needs"""
        out, grad = self._eval(self._tensor(v), True)
        self.terms = out[1:]
        return out[0], grad
