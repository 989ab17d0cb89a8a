"""Isosurface extraction by marching tetrahedra: from a signed distance on a lattice to a triangle mesh, differentiably (kernels: csrc/hip/mtet.hip).

Every other mesh operator of the package works on a fixed topology.  This one is the way back from `signed_distance`, which makes a lattice of signed distances from any
mesh: optimise the values (and, as DMTet does, the positions) of a lattice and extract a mesh at every step, so that handles open and parts merge:

    mt   = psdr.MarchingTetrahedra((nx, ny, nz))
    pos  = psdr.lattice_points((nx, ny, nz), lo, hi)
    topo = mt.extract(sdf)            # MtetTopology(faces, edges, num_vertices, num_faces) on the device; synchronises ONCE, to read the two counts that size the tensors
    v    = mt(sdf, pos)               # [V, 3], differentiable in sdf and pos through the topology of the last extract; no synchronisation
    mesh = mt.to_mesh(v)              # a psdr.Mesh with v attached: gradients of a render reach sdf and pos

The definition is stated once, in include/psdr_hip.h (THE ISOSURFACE).  The lattice has shape (nx, ny, nz) vertices, vertex id u = x + nx (y + ny z), at most 2^24 of them; a
vertex is inside where sdf[u] < 0 (a zero is outside and so is a NaN).  Every cell is split into Kuhn's six tetrahedra; the mesh's vertices are the lattice edges whose ends
differ, in ascending slot order 7 u + c (c: the seven edge classes anchored at u), at p = p_a + t (p_b - p_a), t = s_a / (s_a - s_b) from the anchor; a tetrahedron gives 0, 1
or 2 triangles, wound counter-clockwise seen from outside (SignedDistance's orientation = +1) by a table over (tet, inside mask) - never by a test on pos, so a deformed lattice
keeps the topological orientation.

The gradient holds the topology constant: dp/ds_a = -s_b (p_b - p_a) / (s_a - s_b)^2, dp/ds_b = s_a (p_b - p_a) / (s_a - s_b)^2, dp/dp_a = 1 - t, dp/dp_b = t.  The backward
pass is one gather per lattice vertex over fourteen fixed slots: no sort, no inverted index, no float atomics, the same input gives the same bits.

EXTRACT AT EVERY STEP.  mt(sdf, pos) evaluates the formula on the edges of the LAST extract.  If the signs of sdf have changed since, it still does - with t outside [0, 1] on
the edges that no longer cross - and the mesh is no longer the isosurface.  One GPU only: under an initialised torch.distributed group of more than one rank the calls raise."""
import collections as _collections
import functools as _functools

import numpy as _np

from ._opcommon import MAX_LATTICE, _as_tensor, _ceil_div, _checked_shape, _single_gpu  # noqa: F401

TILE = 256          # entries per workgroup of the scans (csrc/hip/mtet.hip: kThreads)
WAVE = 64

MtetTopology = _collections.namedtuple("MtetTopology", ["faces", "edges", "num_vertices", "num_faces"])
MtetPlan = _collections.namedtuple("MtetPlan", ["tile", "wave", "num_lattice", "num_cells", "vertex_blocks", "cell_blocks", "vertex_passes", "cell_passes", "scratch_ints"])


def launch_plan_mt(shape):
    """How the passes over a lattice of `shape` are split: MtetPlan(tile, wave, num_lattice, num_cells, vertex_blocks, cell_blocks, vertex_passes, cell_passes, scratch_ints),
    a pure function (csrc/hip/mtet.hip: psdr_hip_mtet_plan gives the same numbers).

    The scans are reduce / scan of the workgroup sums / scatter over tiles of `tile` entries, a wave of `wave` lanes scanning by shuffles: vertex_blocks = ceil(Nv / tile)
    workgroups, and vertex_passes = 1 where their sums fit one tile, else 2 (Nv <= 2^24 = tile^3 needs no third); the same for the cells."""
    nx, ny, nz = _checked_shape(shape, "launch_plan_mt")
    nv, nc = nx * ny * nz, (nx - 1) * (ny - 1) * (nz - 1)
    bv, bc = _ceil_div(nv, TILE), _ceil_div(nc, TILE)
    return MtetPlan(TILE, WAVE, nv, nc, bv, bc, 1 if bv <= TILE else 2, 1 if bc <= TILE else 2, 2 * (bv + _ceil_div(bv, TILE)))


def lattice_points(shape, lo=-1.0, hi=1.0):
    """The regular lattice's positions: a float32 [Nv, 3] tensor on the host, row u = x + nx (y + ny z) at lo + (hi - lo) (x / (nx - 1), y / (ny - 1), z / (nz - 1)),
    evaluated in float64 and rounded once.  lo, hi: numbers or three numbers each, hi > lo in every component (a positive spacing: the faces then wind counter-clockwise seen
    from outside)."""
    import torch
    nx, ny, nz = _checked_shape(shape, "lattice_points")
    try:
        lo3, hi3 = (_np.broadcast_to(_np.asarray(q.detach().cpu().numpy() if isinstance(q, torch.Tensor) else q, dtype=_np.float64), (3,)) for q in (lo, hi))
    except (TypeError, ValueError):
        raise ValueError("lattice_points: lo and hi must be numbers or three numbers each, got %r and %r" % (lo, hi)) from None
    if not (_np.isfinite(lo3).all() and _np.isfinite(hi3).all() and (hi3 > lo3).all()):
        raise ValueError("lattice_points: lo and hi must be finite with hi > lo in every component, got %r and %r" % (lo, hi))
    axes = [lo3[a] + (hi3[a] - lo3[a]) * (_np.arange(n, dtype=_np.float64) / (n - 1)) for a, n in enumerate((nx, ny, nz))]
    z, y, x = _np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return torch.from_numpy(_np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(_np.float32))


@_functools.lru_cache(maxsize=None)
def _fn():
    import torch

    class _MtetFn(torch.autograd.Function):
        """mt(sdf, pos): the incoming gradient is a [V, 3] array, so the vector-Jacobian product runs in the backward pass, on the topology the forward pass used"""

        @staticmethod
        def forward(ctx, mt, sdf, pos):
            state = mt._state
            s, p, v = mt._forward(state, sdf, pos)
            ctx.save_for_backward(s, p)
            ctx.mt, ctx.state = mt, state
            ctx.like = ((sdf.device, sdf.dtype), (pos.device, pos.dtype))
            return v

        @staticmethod
        def backward(ctx, g):
            s, p = ctx.saved_tensors
            gs, gp = ctx.mt._adjoint(ctx.state, s, p, g)
            return None, gs.to(*ctx.like[0]) if ctx.needs_input_grad[1] else None, gp.to(*ctx.like[1]) if ctx.needs_input_grad[2] else None

    return _MtetFn


class _State:
    """what a later call needs of an extract: the device, the crossing masks uint8 [Nv], their scan int32 [Nv], and the topology"""

    def __init__(self, device, mask, base, topology):
        self.device, self.mask, self.base, self.topology = device, mask, base, topology
        self.host_faces = None


class MarchingTetrahedra:
    """The isosurface sdf = 0 of a lattice of `shape` = (nx, ny, nz) vertices as a triangle mesh (include/psdr_hip.h has the definition).

    mt.extract(sdf) takes sdf [Nv] on any device and of any float dtype and returns MtetTopology(faces int32 [F, 3], edges int32 [V, 2], num_vertices, num_faces), the tensors
    on the render device: row i of edges is the lattice edge (a, b), a the anchor, that carries mesh vertex i; faces wind counter-clockwise seen from outside.  It synchronises
    once, to read the two counts that size the tensors.  A lattice without a crossing gives empty tensors.  mt.topology keeps the last result.

    mt(sdf, pos) takes pos [Nv, 3] as well and returns the vertices float32 [V, 3] on the render device, on torch's current stream and without a host synchronisation,
    differentiable in both arguments with the topology held constant; the gradients return to the inputs' device and dtype.  It uses the topology of the LAST extract and
    raises before any: extract at every step (the module docstring says what happens otherwise).  mt.vjp(sdf, pos, g) returns (v, g . dv / dsdf [Nv], g . dv / dpos [Nv, 3])
    detached, the same bits as autograd.  mt.to_mesh(v) makes a psdr.Mesh of the last topology with v attached as its vertex_positions."""

    def __init__(self, shape):
        self.shape = _checked_shape(shape, "MarchingTetrahedra")        # checked before a device is looked for
        self.num_lattice = self.shape[0] * self.shape[1] * self.shape[2]
        self.topology = None
        self._state = None

    # ---- arguments

    def _checked_sdf(self, sdf):
        sdf = _as_tensor(sdf)
        if tuple(sdf.shape) != (self.num_lattice,) or not sdf.is_floating_point():
            raise ValueError("MarchingTetrahedra: sdf must be a floating-point [%d] tensor (shape %r), got %s %s" % (self.num_lattice, self.shape, sdf.dtype, tuple(sdf.shape)))
        return sdf

    def _checked_pos(self, pos):
        pos = _as_tensor(pos)
        if tuple(pos.shape) != (self.num_lattice, 3) or not pos.is_floating_point():
            raise ValueError("MarchingTetrahedra: pos must be a floating-point [%d, 3] tensor (shape %r), got %s %s" % (self.num_lattice, self.shape, pos.dtype, tuple(pos.shape)))
        return pos

    def _extracted(self):
        if self._state is None:
            raise RuntimeError("MarchingTetrahedra: no topology yet - call extract(sdf) first (and again whenever the signs of sdf may have changed)")
        return self._state

    @staticmethod
    def _render_device():
        _single_gpu("MarchingTetrahedra")
        from . import _device
        return _device()

    # ---- the passes

    def extract(self, sdf):
        """the topology of sdf's isosurface: MtetTopology(faces, edges, num_vertices, num_faces); one host synchronisation"""
        import torch
        from . import cabi, _stream_ptr
        sdf = self._checked_sdf(sdf)
        device = self._render_device()
        nx, ny, nz = self.shape
        plan = launch_plan_mt(self.shape)
        with torch.cuda.device(device):
            s = sdf.detach().to(device, torch.float32).contiguous()
            mask = torch.empty(plan.num_lattice, device=device, dtype=torch.uint8)
            base = torch.empty(plan.num_lattice, device=device, dtype=torch.int32)
            cell_faces = torch.empty(plan.num_cells, device=device, dtype=torch.uint8)
            cell_base = torch.empty(plan.num_cells, device=device, dtype=torch.int32)
            scratch = torch.empty(plan.scratch_ints, device=device, dtype=torch.int32)
            totals = torch.empty(2, device=device, dtype=torch.int32)
            cabi.check(cabi.lib().psdr_hip_mtet_count(s.data_ptr(), nx, ny, nz, mask.data_ptr(), base.data_ptr(), cell_faces.data_ptr(), cell_base.data_ptr(), scratch.data_ptr(),
                                                      totals.data_ptr(), _stream_ptr()))
            V, F = (int(n) for n in totals.cpu())          # the one synchronisation: the counts size the tensors
            edges = torch.empty((V, 2), device=device, dtype=torch.int32)
            faces = torch.empty((F, 3), device=device, dtype=torch.int32)
            if V > 0 and F > 0:                             # (nothing is launched with an empty grid)
                cabi.check(cabi.lib().psdr_hip_mtet_emit(s.data_ptr(), nx, ny, nz, mask.data_ptr(), base.data_ptr(), cell_base.data_ptr(), V, F, edges.data_ptr(), V,
                                                         faces.data_ptr(), F, _stream_ptr()))
        self.topology = MtetTopology(faces, edges, V, F)
        self._state = _State(device, mask, base, self.topology)
        return self.topology

    def _forward(self, state, sdf, pos):
        """-> (sdf, pos float32 on the device, v [V, 3]), on the current stream"""
        import torch
        from . import cabi, _stream_ptr
        device, V = state.device, state.topology.num_vertices
        nx, ny, nz = self.shape
        with torch.cuda.device(device):
            s, p = sdf.detach().to(device, torch.float32).contiguous(), pos.detach().to(device, torch.float32).contiguous()
            v = torch.empty((V, 3), device=device, dtype=torch.float32)
            if V > 0:
                cabi.check(cabi.lib().psdr_hip_mtet_vertices(s.data_ptr(), p.data_ptr(), nx, ny, nz, state.topology.edges.data_ptr(), V, v.data_ptr(), _stream_ptr()))
        return s, p, v

    def _adjoint(self, state, s, p, g):
        """the vector-Jacobian product for g [V, 3] -> (gs [Nv], gp [Nv, 3]) on the device, on the current stream"""
        import torch
        from . import cabi, _stream_ptr
        device, V = state.device, state.topology.num_vertices
        nx, ny, nz = self.shape
        with torch.cuda.device(device):
            if V == 0:
                return torch.zeros_like(s), torch.zeros_like(p)
            g = g.detach().to(device, torch.float32).contiguous()
            gs, gp = torch.empty_like(s), torch.empty_like(p)
            cabi.check(cabi.lib().psdr_hip_mtet_vertices_adj(s.data_ptr(), p.data_ptr(), nx, ny, nz, state.mask.data_ptr(), state.base.data_ptr(), V, g.data_ptr(),
                                                             gs.data_ptr(), gp.data_ptr(), _stream_ptr()))
        return gs, gp

    def __call__(self, sdf, pos):
        """the mesh's vertices, a float32 [V, 3] tensor, through the topology of the last extract"""
        sdf, pos = self._checked_sdf(sdf), self._checked_pos(pos)
        self._extracted()
        return _fn().apply(self, sdf, pos)

    def vjp(self, sdf, pos, g):
        """(v, g . dv / dsdf, g . dv / dpos) without autograd, all detached on the render device: what a hand-written adjoint needs.  g: [V, 3], any device, any float dtype"""
        sdf, pos = self._checked_sdf(sdf), self._checked_pos(pos)
        state = self._extracted()
        g = _as_tensor(g)
        if tuple(g.shape) != (state.topology.num_vertices, 3) or not g.is_floating_point():
            raise ValueError("MarchingTetrahedra: g must be a floating-point [%d, 3] tensor, got %s %s" % (state.topology.num_vertices, g.dtype, tuple(g.shape)))
        s, p, v = self._forward(state, sdf, pos)
        gs, gp = self._adjoint(state, s, p, g)
        return v, gs, gp

    def to_mesh(self, v):
        """a psdr.Mesh of the last topology: load_raw(v, faces) with `v` attached as vertex_positions, so that gradients of a render reach sdf and pos through v.  The faces
        come to the host once per extract (a copy that waits).  A new topology is a new mesh, in a new or rebuilt scene."""
        import torch
        from . import Mesh
        state = self._extracted()
        V, F = state.topology.num_vertices, state.topology.num_faces
        v = _as_tensor(v)
        if tuple(v.shape) != (V, 3) or not v.is_floating_point():
            raise ValueError("to_mesh: expected a floating-point [%d, 3] tensor, got %s %s" % (V, v.dtype, tuple(v.shape)))
        if F == 0:
            raise ValueError("to_mesh: the last extract found no face")
        if state.host_faces is None:
            state.host_faces = _np.ascontiguousarray(state.topology.faces.cpu().numpy(), _np.int32)
        m = Mesh()
        m.load_raw(v.detach().to("cpu", torch.float32).numpy(), state.host_faces, _np.zeros((0, 2), _np.float32), _np.zeros((0, 3), _np.int32))
        m.vertex_positions = v
        return m
