"""Loop / midpoint mesh subdivision as a differentiable operator on per-vertex arrays ("Large Steps in Inverse Rendering", Nicolet et al. 2021, section 5:
coarse to fine).

    sub = psdr.Subdivision(cage_mesh, levels=2)                         # the cage is the parameter: render v = S c, c.grad = S^T v.grad
    fine = sub.to_mesh(sub.refine(c)); sc.add_Mesh(fine, "mat", None)
    # each step:  sc.param_map["Mesh[k]"].vertex_positions = sub.refine(c); sc.configure(); loss(renderD(...)).backward()

    sub = psdr.Subdivision(mesh, levels=1, scheme="linear")             # a stage change: the same surface, four times the faces
    fine = sub.to_mesh(sub.refine(V), sub.refine_uv(UV)); pre = psdr.LaplacianPreconditioner(sub.faces, sub.num_vertices_out)

The topology is numpy and runs once per mesh and level on the host (subdivision_level, usable without the native library): the fine faces, the
matrix S with its float32 weights, and S^T as a second CSR with the very same values.  The products run in libpsdr_hip.so
(psdr_hip_subdiv_apply / psdr_hip_subdiv_apply_adj, csrc/hip/subdiv.hip): one gather kernel for both directions, one launch per level, no atomics -
the same input gives the same bits, forward and backward.
"""
import collections as _collections
import ctypes as _C
import functools as _functools

import numpy as _np

SCHEMES = ("loop", "linear")

SubdivisionLevel = _collections.namedtuple("SubdivisionLevel", [
    "faces",                # int32 [4 F, 3]: face f's children are 4 f .. 4 f + 3
    "num_vertices_in", "num_vertices_out", "num_edges", "num_sharp_edges",
    "row_begin", "col", "weight",               # S   [n_out x n_in]: int32 [n_out + 1], int32 [nnz], float32 [nnz]; ascending columns in every row
    "t_row_begin", "t_col", "t_weight",         # S^T [n_in x n_out], the same float32 values
])


def _faces_checked(faces, n, what):
    f = _np.asarray(faces)
    if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] == 0:
        raise ValueError("%s must be [f, 3] with f >= 1, got shape %s" % (what, tuple(f.shape)))
    if not _np.issubdtype(f.dtype, _np.integer):
        raise ValueError("%s must hold integer ids" % what)
    f = f.astype(_np.int64)
    if n <= 0:
        raise ValueError("%s: the number of vertices must be positive" % what)
    if f.min() < 0 or f.max() >= n:
        raise ValueError("%s: an id is outside [0, %d)" % (what, n))
    bad = _np.nonzero((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0]))[0]
    if bad.size:
        raise ValueError("%s: face %d repeats a vertex id: %s" % (what, int(bad[0]), f[bad[0]].tolist()))
    return f


def subdivision_level(faces, num_vertices, scheme="loop"):
    """One level of subdivision of a triangle list: a SubdivisionLevel (fine faces, n_out, S and S^T as CSR).  Host-side numpy, no GPU.

    faces [F, 3] vertex ids in [0, n), n = num_vertices; a face with a repeated id or an id out of range is a ValueError.

    Edges: the distinct undirected vertex pairs, numbered e = 0 .. E - 1 in ascending (min id, max id) order; m_e = the number of faces at edge e (a
    duplicate face counts twice).  m_e == 2: interior, with opposite vertices o0, o1; anything else (boundary m_e == 1, non-manifold m_e >= 3): sharp.
    Vertices: d_v distinct edges at v, s_v of them sharp.  d_v == 0: unused, identity row; s_v == 0: smooth, Warren's weights (beta = 3/16 if d_v == 3
    else 3 / (8 d_v); 1 - d_v beta on itself, beta on each neighbour); s_v == 2: crease, 3/4 on itself and 1/8 on the other end of each of its two sharp
    edges; anything else: corner, identity row.
    Fine vertex i < n is coarse vertex i (ids persist); fine vertex n + e is edge e's: 3/8 on each end and 1/8 on o0 and on o1 for an interior edge,
    1/2 on each end for a sharp one.  scheme="linear": identity rows and 1/2, 1/2 - the surface does not move.
    Face (a, b, c) with edge vertices ab, bc, ca becomes (a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca), in this order; orientation is kept.

    There is no vertex welding: a seam that an OBJ file lists twice is a boundary here and becomes a crease.  Weld the mesh first where that matters.

    The weights are formed in float64 and rounded to float32 once, here; entries that fall on the same column (o0 == o1: two faces over the same three
    vertices) are one entry with the sum.  S^T holds the very same float32 values."""
    if scheme not in SCHEMES:
        raise ValueError("unknown subdivision scheme %r (one of %s)" % (scheme, ", ".join(SCHEMES)))
    n = int(num_vertices)
    f = _faces_checked(faces, n, "faces")
    F = f.shape[0]
    # the three half-edges of every face: block 0 is (a, b), block 1 (b, c), block 2 (c, a); `opp` the face's third vertex
    ha = _np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    hb = _np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    opp = _np.concatenate([f[:, 2], f[:, 0], f[:, 1]])
    key, edge_of, m = _np.unique(_np.minimum(ha, hb) * n + _np.maximum(ha, hb), return_inverse=True, return_counts=True)
    edge_of = edge_of.reshape(-1)
    E = int(key.size)
    lo, hi = key // n, key % n
    n_out = n + E
    if 4 * n_out >= 2 ** 31:
        raise ValueError("subdivision_level: %d fine vertices: 4 n_out must stay below 2^31" % n_out)
    interior = m == 2
    eid = _np.arange(E, dtype=_np.int64)
    ident = _np.arange(n, dtype=_np.int64)
    if scheme == "linear":
        rows = [ident, n + eid, n + eid]
        cols = [ident, lo, hi]
        vals = [_np.ones(n), _np.full(E, 0.5), _np.full(E, 0.5)]
    else:
        by_edge = _np.argsort(edge_of, kind="stable")          # the half-edges grouped by edge, in face order inside a group
        first = _np.concatenate([[0], _np.cumsum(m)[:-1]])
        ie = eid[interior]
        o0, o1 = opp[by_edge[first[interior]]], opp[by_edge[first[interior] + 1]]
        se = eid[~interior]
        d = _np.bincount(lo, minlength=n) + _np.bincount(hi, minlength=n)
        s = _np.bincount(lo[se], minlength=n) + _np.bincount(hi[se], minlength=n)
        smooth = (d > 0) & (s == 0)
        crease = (d > 0) & (s == 2)
        fixed = ~(smooth | crease)                              # unused and corner vertices
        beta = _np.where(d == 3, 3.0 / 16.0, 3.0 / (8.0 * _np.maximum(d, 1)))
        # the edges seen from both of their ends: (vertex, the other end, sharp?)
        ev, eo, es = _np.concatenate([lo, hi]), _np.concatenate([hi, lo]), _np.concatenate([~interior, ~interior])
        ring = smooth[ev]
        side = crease[ev] & es
        sv, cv, fv = ident[smooth], ident[crease], ident[fixed]
        rows = [fv, sv, ev[ring], cv, ev[side], n + ie, n + ie, n + ie, n + ie, n + se, n + se]
        cols = [fv, sv, eo[ring], cv, eo[side], lo[ie], hi[ie], o0, o1, lo[se], hi[se]]
        vals = [_np.ones(fv.size), 1.0 - d[sv] * beta[sv], beta[ev[ring]], _np.full(cv.size, 0.75), _np.full(int(side.sum()), 0.125),
                _np.full(ie.size, 0.375), _np.full(ie.size, 0.375), _np.full(ie.size, 0.125), _np.full(ie.size, 0.125),
                _np.full(se.size, 0.5), _np.full(se.size, 0.5)]
    r, c, v = _np.concatenate(rows), _np.concatenate(cols), _np.concatenate(vals).astype(_np.float64)
    order = _np.lexsort((c, r))
    r, c, v = r[order], c[order], v[order]
    head = _np.ones(r.size, dtype=bool)
    head[1:] = (r[1:] != r[:-1]) | (c[1:] != c[:-1])            # entries on the same (row, column) become one
    starts = _np.nonzero(head)[0]
    v = _np.add.reduceat(v, starts)
    r, c = r[starts], c[starts]
    w = v.astype(_np.float32)
    if r.size >= 2 ** 31:
        raise ValueError("subdivision_level: more than 2^31 - 1 entries")
    row_begin = _np.zeros(n_out + 1, dtype=_np.int64)
    _np.cumsum(_np.bincount(r, minlength=n_out), out=row_begin[1:])
    t_order = _np.lexsort((r, c))                                # the inverted index: by column, then by row
    t_row_begin = _np.zeros(n + 1, dtype=_np.int64)
    _np.cumsum(_np.bincount(c, minlength=n), out=t_row_begin[1:])
    e_ab, e_bc, e_ca = n + edge_of[:F], n + edge_of[F:2 * F], n + edge_of[2 * F:]
    a, b, cc = f[:, 0], f[:, 1], f[:, 2]
    fine = _np.stack([_np.stack([a, e_ab, e_ca], 1), _np.stack([b, e_bc, e_ab], 1), _np.stack([cc, e_ca, e_bc], 1), _np.stack([e_ab, e_bc, e_ca], 1)], 1)
    i32 = _np.int32
    return SubdivisionLevel(_np.ascontiguousarray(fine.reshape(4 * F, 3).astype(i32)), n, n_out, E, int((~interior).sum()),
                            row_begin.astype(i32), c.astype(i32), w,
                            t_row_begin.astype(i32), r[t_order].astype(i32), _np.ascontiguousarray(w[t_order]))


class _Handle:
    """owner of a psdr_hip_subdiv: one level's S and S^T on the device"""

    def __init__(self, lv, stream):
        from . import cabi
        self._cabi = cabi
        self.ptr = _C.c_void_p()
        arrays = [_np.ascontiguousarray(a, t) for a, t in ((lv.row_begin, _np.int32), (lv.col, _np.int32), (lv.weight, _np.float32),
                                                           (lv.t_row_begin, _np.int32), (lv.t_col, _np.int32), (lv.t_weight, _np.float32))]
        cabi.check(cabi.lib().psdr_hip_subdiv_create(int(lv.num_vertices_in), int(lv.num_vertices_out), *[a.ctypes.data for a in arrays], _C.byref(self.ptr), stream))

    def __del__(self):
        if getattr(self, "ptr", None) and getattr(self, "_cabi", None) is not None and self._cabi.lib is not None:
            self._cabi.lib().psdr_hip_subdiv_destroy(self.ptr)
            self.ptr = None


@_functools.lru_cache(maxsize=None)
def _fn():
    """the autograd function, made on first use: subdivision_level() needs neither torch nor the native library"""
    import torch

    class _ChainFn(torch.autograd.Function):
        """y = S_L .. S_1 x (adjoint False) or (S_L .. S_1)^T x (True); the backward is the other direction"""

        @staticmethod
        def forward(ctx, sub, uv, adjoint, x):
            ctx.sub, ctx.uv, ctx.adjoint, ctx.like = sub, uv, adjoint, (x.device, x.dtype)
            return sub._run(x, uv, adjoint)

        @staticmethod
        def backward(ctx, g):
            return None, None, None, ctx.sub._run(g, ctx.uv, not ctx.adjoint).to(*ctx.like)

    return _ChainFn


class Subdivision:
    """`levels` levels of Loop (scheme="loop") or midpoint (scheme="linear") subdivision of one mesh, as a linear operator on per-vertex arrays.

    mesh_or_faces: a Mesh (its face_indices / num_vertices and, when it has uv, face_uv_indices / vertex_uv are read) or a [f, 3] array of vertex
    ids with `num_vertices`; face_uv [f, 3] and num_uv give a uv index topology with a face array.  The rules are subdivision_level()'s; level
    l + 1 is built from level l's fine faces.  The uv set is refined over its OWN index topology and always by the midpoint rule, with the same
    child order, so that fine face k's position and uv indices describe the same corners and a texture lookup on the fine mesh equals the lookup on
    the coarse triangle.  No vertex welding: a seam the file lists twice is a boundary and becomes a crease under "loop".

    refine(c) = S_L .. S_1 c takes [num_vertices_in, C], C in 1 .. 4, on any device and of any float dtype, and returns float32
    [num_vertices_out, C] on the render device, computed on torch's current stream; restrict(y) = (S_L .. S_1)^T y goes the other way.  Both are
    differentiable, each the other's backward, and gradients return to the input's device and dtype.  refine_uv / restrict_uv are the uv topology's
    operator.  One launch per level and direction; no composite matrix is formed.  No atomics: the same input gives the same bits.  One GPU."""

    def __init__(self, mesh_or_faces, num_vertices=None, levels=1, scheme="loop", face_uv=None, num_uv=None):
        if scheme not in SCHEMES:
            raise ValueError("Subdivision: unknown scheme %r (one of %s)" % (scheme, ", ".join(SCHEMES)))
        if int(levels) != levels or int(levels) < 1:
            raise ValueError("Subdivision: levels must be an integer >= 1, got %r" % (levels,))
        if hasattr(mesh_or_faces, "face_indices") and hasattr(mesh_or_faces, "num_vertices"):
            mesh = mesh_or_faces
            faces = _np.asarray(mesh.face_indices).reshape(-1, 3)
            num_vertices = int(mesh.num_vertices) if num_vertices is None else int(num_vertices)
            if face_uv is None and _np.asarray(mesh.face_uv_indices).size:
                face_uv = _np.asarray(mesh.face_uv_indices).reshape(-1, 3)
                num_uv = _np.asarray(mesh.vertex_uv).reshape(-1, 2).shape[0] if num_uv is None else num_uv
        else:
            faces = _np.asarray(mesh_or_faces)
            if num_vertices is None:
                raise ValueError("Subdivision: num_vertices is required with a face array")
        if face_uv is not None:
            face_uv = _np.asarray(face_uv)
            if num_uv is None:
                raise ValueError("Subdivision: num_uv is required with face_uv")
            if face_uv.ndim != 2 or faces.ndim != 2 or face_uv.shape != faces.shape:
                raise ValueError("Subdivision: face_uv %s must have the shape of faces %s" % (tuple(face_uv.shape), tuple(faces.shape)))
        self.levels, self.scheme = int(levels), scheme
        self._pos, self._uv = [], []
        f, n = faces, int(num_vertices)
        for _ in range(self.levels):
            lv = subdivision_level(f, n, scheme)
            self._pos.append(lv)
            f, n = lv.faces, lv.num_vertices_out
        self.num_vertices_in, self.num_vertices_out, self.faces = self._pos[0].num_vertices_in, n, f
        self.num_uv_in = self.num_uv_out = self.face_uv = None
        if face_uv is not None:
            f, n = _faces_checked(face_uv, int(num_uv), "face_uv"), int(num_uv)
            for _ in range(self.levels):
                lv = subdivision_level(f, n, "linear")
                self._uv.append(lv)
                f, n = lv.faces, lv.num_vertices_out
            self.num_uv_in, self.num_uv_out, self.face_uv = self._uv[0].num_vertices_in, n, f
        from . import _device, _stream_ptr
        import torch
        self._device = _device()
        with torch.cuda.device(self._device):
            self._handles = {False: [_Handle(lv, _stream_ptr()) for lv in self._pos], True: [_Handle(lv, _stream_ptr()) for lv in self._uv]}

    def _run(self, x, uv, adjoint):
        """the chain on the device: x [rows, C] -> float32 [rows', C] on the render device, one launch per level"""
        import torch
        from . import cabi, _stream_ptr
        lvs, handles = (self._uv, self._handles[True]) if uv else (self._pos, self._handles[False])
        if uv and not lvs:
            raise ValueError("Subdivision: the mesh has no uv set")
        rows = lvs[-1].num_vertices_out if adjoint else lvs[0].num_vertices_in
        if x.dim() != 2 or x.shape[0] != rows or not 1 <= x.shape[1] <= 4:
            raise ValueError("expected a [%d, C] tensor with C in 1 .. 4, got %s" % (rows, tuple(x.shape)))
        if not x.is_floating_point():
            raise ValueError("expected a floating-point tensor, got %s" % x.dtype)
        C = int(x.shape[1])
        x = x.detach().to(self._device, torch.float32).contiguous()
        L = cabi.lib()
        with torch.cuda.device(self._device):
            for lv, h in (zip(reversed(lvs), reversed(handles)) if adjoint else zip(lvs, handles)):
                y = torch.empty((lv.num_vertices_in if adjoint else lv.num_vertices_out, C), device=self._device, dtype=torch.float32)
                cabi.check((L.psdr_hip_subdiv_apply_adj if adjoint else L.psdr_hip_subdiv_apply)(h.ptr, x.data_ptr(), C, y.data_ptr(), _stream_ptr()))
                x = y
        return x

    @staticmethod
    def _tensor(x):
        import torch
        return x if isinstance(x, torch.Tensor) else torch.as_tensor(_np.asarray(x))

    def refine(self, c):
        """v = S_L .. S_1 c: [num_vertices_in, C] -> [num_vertices_out, C]"""
        return _fn().apply(self, False, False, self._tensor(c))

    def restrict(self, y):
        """g = (S_L .. S_1)^T y: [num_vertices_out, C] -> [num_vertices_in, C]"""
        return _fn().apply(self, False, True, self._tensor(y))

    def refine_uv(self, uv0):
        """the uv topology's (always midpoint) operator: [num_uv_in, C] -> [num_uv_out, C]"""
        return _fn().apply(self, True, False, self._tensor(uv0))

    def restrict_uv(self, y):
        """its transpose: [num_uv_out, C] -> [num_uv_in, C]"""
        return _fn().apply(self, True, True, self._tensor(y))

    def csr(self, level, transpose=False, uv=False):
        """(row_begin, col, weight) of level `level` (0-based) as numpy arrays: what the device holds.  transpose: S^T; uv: the uv topology's"""
        lvs = self._uv if uv else self._pos
        if uv and not lvs:
            raise ValueError("Subdivision: the mesh has no uv set")
        if not 0 <= int(level) < len(lvs):
            raise ValueError("Subdivision: level %r is outside [0, %d)" % (level, len(lvs)))
        lv = lvs[int(level)]
        return (lv.t_row_begin, lv.t_col, lv.t_weight) if transpose else (lv.row_begin, lv.col, lv.weight)

    def to_mesh(self, v, uv=None):
        """a psdr.Mesh of the fine topology: load_raw(v, faces, uv, face_uv), with `v` attached as vertex_positions so that gradients reach it"""
        import torch
        from . import Mesh
        v = self._tensor(v)
        if tuple(v.shape) != (self.num_vertices_out, 3):
            raise ValueError("to_mesh: expected a [%d, 3] tensor, got %s" % (self.num_vertices_out, tuple(v.shape)))
        if uv is not None:
            if self.face_uv is None:
                raise ValueError("to_mesh: the mesh has no uv set")
            uv = self._tensor(uv)
            if tuple(uv.shape) != (self.num_uv_out, 2):
                raise ValueError("to_mesh: expected a [%d, 2] uv tensor, got %s" % (self.num_uv_out, tuple(uv.shape)))
            uv_np = uv.detach().to("cpu", torch.float32).numpy()
        m = Mesh()
        if uv is None:
            m.load_raw(v.detach().to("cpu", torch.float32).numpy(), self.faces, _np.zeros((0, 2), _np.float32), _np.zeros((0, 3), _np.int32))
        else:
            m.load_raw(v.detach().to("cpu", torch.float32).numpy(), self.faces, uv_np, self.face_uv)
        m.vertex_positions = v
        return m
