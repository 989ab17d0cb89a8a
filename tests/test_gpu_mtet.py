"""GPU tests of marching tetrahedra (psdr_jit_amd/mtet.py, csrc/hip/mtet.hip) against the numpy statement of the definition in tests/mtet_ref.py.

The topology is exact: edges must equal the checker's bit for bit and faces must equal it as canonical sets (every triangle rotated so that its smallest index comes first, rows
sorted) - on all 256 sign patterns of one cell (every row of the kernel's (tet, mask) table, orientation included), on lattices whose strides differ, and on shapes read from
launch_plan_mt whose vertex and cell counts straddle every boundary of the scans (a wave, a workgroup, one pass of workgroup sums), plus 33^3 with random signs.  Positions and
both vector-Jacobian products follow the rule of tests/test_gpu_meshreg.py: e_gpu <= 4 max(e_32, u G), u = 2^-24, G the largest magnitude of the array, e_32 the error of the
float32 checker against float64.  Then the exact cases (t in {1/2, 1/4, 3/4} bit for bit, zeros on a plane, NaN, no crossing), the round trip through winding_number,
repeatability, both stream forms of tests/stream_cases.py, autograd, and a render whose gradient reaches the lattice's values.

Measured on an MI355X, the worst e_gpu / max(e_32, u G) over all cases: v 0.93 (the sphere), d / dsdf 1.00, d / dpos 1.00 - the float32 checker's own
error: the device has the checker's operations in the checker's order."""
import os

import numpy as np
import pytest

import mtet_ref as ref
import scenes
from stream_cases import Slot, run_on_stream, run_plain

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def psdr():
    import __graft_entry__
    __graft_entry__.build()
    import psdr_jit_amd
    return psdr_jit_amd


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a))


def _np(t):
    return t.cpu().numpy()


def _held(what, worst, key, dev, f32, f64):
    r, e_gpu, e_32, G = ref.ratio(dev, f32, f64)
    worst[key] = max(worst.get(key, 0.0), r)
    assert np.isfinite(np.asarray(dev)).all(), what
    assert r <= 4.0, "%s, %s: e_gpu = %.3g, e_32 = %.3g, u G = %.3g: ratio %.3g > 4" % (what, key, e_gpu, e_32, ref.U * G, r)


def _report(what, worst):
    print("%s: worst e_gpu / max(e_32, u G): %s" % (what, ", ".join("%s %.2f" % kv for kv in sorted(worst.items()))))


def _same_topology(what, topo, r):
    """the device's topology is the checker's: the counts, edges bit for bit, faces as canonical sets"""
    import torch
    V, F = len(r["edges"]), len(r["faces"])
    assert (topo.num_vertices, topo.num_faces) == (V, F), "%s: (V, F) = (%d, %d), the checker has (%d, %d)" % (what, topo.num_vertices, topo.num_faces, V, F)
    assert topo.edges.dtype == torch.int32 and topo.faces.dtype == torch.int32 and topo.edges.is_cuda and topo.faces.is_cuda
    assert tuple(topo.edges.shape) == (V, 2) and tuple(topo.faces.shape) == (F, 3)
    assert np.array_equal(_np(topo.edges), r["edges"]), what
    assert np.array_equal(ref.canonical(_np(topo.faces)), ref.canonical(r["faces"])), what


def _random_signs(shape, seed):
    return np.random.default_rng(seed).choice(np.array([-1.0, 1.0], np.float32), ref.counts(shape)[0])


# ---- 1. one cell

def test_one_cell_all_256_patterns(psdr):
    mt = psdr.MarchingTetrahedra((2, 2, 2))
    faces = 0
    for pattern in range(256):
        sdf = np.where(pattern >> np.arange(8) & 1, -1.0, 1.0).astype(np.float32)
        topo = mt.extract(_t(sdf))
        _same_topology("pattern %d" % pattern, topo, ref.topology(sdf, (2, 2, 2)))
        assert (topo.num_faces == 0) == (pattern in (0, 255))
        faces += topo.num_faces
    assert faces > 256


# ---- 2. strides

@pytest.mark.parametrize("shape", [(2, 3, 5), (5, 3, 2)])
def test_strides(psdr, shape):
    """extents that all differ: a swapped extent or a wrong boundary slot of any class changes the topology"""
    worst = {}
    sdf, pos = ref.random_sdf(shape, 11), ref.jittered(shape, 12)
    mt = psdr.MarchingTetrahedra(shape)
    topo = mt.extract(_t(sdf))
    r = ref.topology(sdf, shape)
    _same_topology(str(shape), topo, r)
    edges = _np(topo.edges)                                       # positions and products through the device's topology
    g = np.random.default_rng(13).uniform(-1, 1, (len(edges), 3)).astype(np.float32)
    v, gs, gp = mt.vjp(_t(sdf), _t(pos), _t(g))
    _held(str(shape), worst, "v", _np(v), ref.positions(sdf, pos, edges, np.float32), ref.positions(sdf, pos, edges))
    gs32, gp32 = ref.vjp(sdf, pos, edges, g, shape, np.float32)
    gs64, gp64 = ref.vjp(sdf, pos, edges, g, shape)
    _held(str(shape), worst, "grad_sdf", _np(gs), gs32, gs64)
    _held(str(shape), worst, "grad_pos", _np(gp), gp32, gp64)
    _report("strides %s" % (shape,), worst)


# ---- 3. the plan's boundaries

def _boundary_shapes(psdr, which):
    """three shapes (nx, ny - 1 | ny | ny + 1, 2) around a boundary of the scans, read from the plan: `which` = (vertices | cells, wave | tile | pass)"""
    over, edge = which
    plan = psdr.launch_plan_mt((2, 2, 2))
    B = {"wave": plan.wave, "tile": plan.tile, "pass": plan.tile * plan.tile}[edge]
    count = B // 2 if over == "vertices" else B                  # vertices: nx ny 2 = B; cells: (nx - 1) (ny - 1) 1 = B
    a = 1 << ((count.bit_length() - 1 + 1) // 2)
    b = count // a
    assert a * b == count
    nx, ny = (a, b) if over == "vertices" else (a + 1, b + 1)
    shapes = [(nx, ny - 1, 2), (nx, ny, 2), (nx, ny + 1, 2)]
    plans = [psdr.launch_plan_mt(s) for s in shapes]
    n = [p.num_lattice if over == "vertices" else p.num_cells for p in plans]
    assert n[0] < B == n[1] < n[2]                                # below by one row, on the boundary, above by one row
    blocks = [p.vertex_blocks if over == "vertices" else p.cell_blocks for p in plans]
    passes = [p.vertex_passes if over == "vertices" else p.cell_passes for p in plans]
    if edge == "tile":
        assert blocks == [1, 1, 2]
    if edge == "pass":
        assert blocks[1] == plan.tile < blocks[2] and passes == [1, 1, 2]
    return shapes


@pytest.mark.parametrize("which", [(o, e) for o in ("vertices", "cells") for e in ("wave", "tile", "pass")], ids=lambda w: "%s-%s" % w)
def test_shapes_on_the_edges_of_the_plan(psdr, which):
    """random signs: about half of all slots cross; the topology and the counts are the checker's below, on and above every boundary"""
    for k, shape in enumerate(_boundary_shapes(psdr, which)):
        sdf = _random_signs(shape, 20 + k)
        topo = psdr.MarchingTetrahedra(shape).extract(_t(sdf))
        _same_topology("%s %s" % (which, shape), topo, ref.topology(sdf, shape))


def test_33_cubed_with_random_signs(psdr):
    """the worst case: about half of all slots cross, both scans in two levels of workgroups"""
    shape = (33, 33, 33)
    plan = psdr.launch_plan_mt(shape)
    assert plan.vertex_blocks > 1 and plan.cell_blocks > 1 and plan.num_lattice % plan.tile != 0
    sdf = _random_signs(shape, 30)
    topo = psdr.MarchingTetrahedra(shape).extract(_t(sdf))
    r = ref.topology(sdf, shape)
    assert 0.4 * 7 * plan.num_lattice < len(r["edges"]) < 0.5 * 7 * plan.num_lattice
    _same_topology("33^3", topo, r)


# ---- 4. exact cases

def test_quarter_points_are_bit_equal(psdr):
    """the integer lattice with values in {-1, 1, 3, -3}: t is 1 / 2, 1 / 4 or 3 / 4 and every position is exact"""
    shape = (6, 5, 4)
    sdf = np.random.default_rng(40).choice(np.array([-1.0, 1.0, 3.0, -3.0], np.float32), ref.counts(shape)[0])
    pos = ref.coords(shape).astype(np.float32)
    mt = psdr.MarchingTetrahedra(shape)
    topo = mt.extract(_t(sdf))
    r = ref.reference(sdf, pos, shape)
    _same_topology("quarters", topo, r)
    v = _np(mt(_t(sdf), _t(pos)))
    frac = np.unique((v - np.floor(v)).round(6))
    assert set(frac.tolist()) <= {0.0, 0.25, 0.5, 0.75} and {0.25, 0.5, 0.75} <= set(frac.tolist())
    assert _bits(v) == _bits(r["v32"]) and np.array_equal(r["v32"], r["v64"])


def test_zeros_on_a_plane_nan_and_no_crossing(psdr):
    import torch
    shape = (5, 3, 3)
    X = ref.coords(shape)
    pos = X.astype(np.float32)
    mt = psdr.MarchingTetrahedra(shape)
    # sdf = x - 2: zeros on a whole plane count as outside, the coincident vertices are present
    sdf = (X[:, 0] - 2).astype(np.float32)
    r = ref.reference(sdf, pos, shape)
    topo = mt.extract(_t(sdf))
    _same_topology("x - 2", topo, r)
    v = _np(mt(_t(sdf), _t(pos)))
    assert np.isfinite(v).all() and _bits(v) == _bits(r["v32"]) and (v[:, 0] == 2).all() and len(np.unique(v, axis=0)) < len(v)
    g = np.ones_like(v)
    _v, gs, gp = mt.vjp(_t(sdf), _t(pos), _t(g))
    assert np.isfinite(_np(gs)).all() and np.isfinite(_np(gp)).all()
    # NaN is outside
    nan = ref.random_sdf(shape, 41)
    nan[np.random.default_rng(42).choice(len(nan), 9, replace=False)] = np.nan
    assert np.isnan(nan).sum() == 9
    _same_topology("nan", mt.extract(_t(nan)), ref.topology(nan, shape))
    # no crossing: empty outputs, mt(...) gives [0, 3]
    for value in (1.0, -1.0, 0.0):
        flat = np.full(len(sdf), value, np.float32)
        topo = mt.extract(_t(flat))
        assert (topo.num_vertices, topo.num_faces) == (0, 0) and tuple(topo.edges.shape) == (0, 2) and tuple(topo.faces.shape) == (0, 3)
        assert topo.edges.dtype == torch.int32 and topo.faces.dtype == torch.int32
        out = mt(_t(flat), _t(pos))
        assert tuple(out.shape) == (0, 3) and out.dtype == torch.float32 and out.is_cuda
        v0, gs0, gp0 = mt.vjp(_t(flat), _t(pos), torch.zeros(0, 3))
        assert tuple(v0.shape) == (0, 3) and not _np(gs0).any() and not _np(gp0).any() and tuple(gp0.shape) == (len(sdf), 3)
        s = _t(flat).requires_grad_()
        mt(s, _t(pos)).sum().backward()
        assert s.grad is not None and not s.grad.any()


# ---- 5. the round trip through the signed distance

def test_round_trip_through_the_winding_number(psdr):
    """the extracted sphere's winding number says inside exactly where the lattice's values are negative, and its vertices lie within a cell diagonal of the sphere"""
    shape = ref.SPHERE_SHAPE
    pos, sdf = ref.sphere()
    assert np.abs(sdf).min() >= 1e-3
    mt = psdr.MarchingTetrahedra(shape)
    topo = mt.extract(_t(sdf))
    r = ref.reference(sdf, pos, shape, key="sphere")
    _same_topology("sphere", topo, r)
    v = mt(_t(sdf), _t(pos))
    worst = {}
    _held("sphere", worst, "v", _np(v), r["v32"], r["v64"])
    _report("sphere", worst)
    w = _np(psdr.winding_number(_t(pos), v, topo.faces))
    assert np.array_equal(w > 0.5, sdf < 0) and (sdf < 0).sum() > 50
    off = np.abs(np.linalg.norm(_np(v).astype(np.float64) - ref.SPHERE_CENTRE, axis=1) - ref.SPHERE_RADIUS)
    assert off.max() < ref.cell_diagonal(shape)
    assert psdr.lattice_points(shape, -1.0, 1.0).numpy().tobytes() == pos.tobytes()


# ---- 6. repeatability, streams

def _case(shape=(9, 8, 7), seed=50):
    sdf, pos = ref.random_sdf(shape, seed), ref.jittered(shape, seed + 1)
    return shape, sdf, pos


def test_two_calls_return_identical_bytes(psdr):
    shape, sdf, pos = _case((17, 16, 15), 52)
    mt = psdr.MarchingTetrahedra(shape)
    runs = []
    for _ in range(2):
        topo = mt.extract(_t(sdf))
        g = _t(np.random.default_rng(54).uniform(-1, 1, (topo.num_vertices, 3)).astype(np.float32))
        v, gs, gp = mt.vjp(_t(sdf), _t(pos), g)
        runs.append(tuple(_bits(_np(a)) for a in (topo.edges, topo.faces, v, gs, gp)))
    assert runs[0] == runs[1] and all(len(b) > 0 for b in runs[0])


@pytest.mark.parametrize("form", ("S", "default"))
def test_streams(psdr, form):
    """both forms of the delayed producer: extract (it reads the counts, so it cannot return early) and mt(...) / vjp (they do); sdf and pos rolled along their first axis
    are the decoys"""
    import torch
    shape, sdf, pos = _case()
    mt = psdr.MarchingTetrahedra(shape)
    ss, sp = Slot(torch, sdf), Slot(torch, pos)
    fetch = lambda out: tuple(_np(a) for a in out)
    r = ref.topology(sdf, shape)
    g = _t(np.random.default_rng(55).uniform(-1, 1, (len(r["edges"]), 3)).astype(np.float32)).cuda()
    assert not np.array_equal(ref.topology(ss._decoy.cpu().numpy(), shape)["edges"], r["edges"])          # the decoy is told apart
    S = torch.cuda.Stream()

    def extract():
        topo = mt.extract(ss.buf)
        return (topo.edges, topo.faces)
    got = run_on_stream(torch, S, form, [ss], extract, fetch, returns_early=False)
    assert np.array_equal(got[0], r["edges"]) and np.array_equal(ref.canonical(got[1]), ref.canonical(r["faces"]))
    # the topology of the true input stays; the positions and the products return without a synchronisation
    base = run_plain(torch, [ss, sp], lambda: mt.vjp(ss.buf, sp.buf, g), fetch)
    assert _bits(_np(mt.vjp(ss._decoy, sp.buf, g)[0])) != _bits(base[0]) and _bits(_np(mt.vjp(ss.buf, sp._decoy, g)[0])) != _bits(base[0])
    got = run_on_stream(torch, S, form, [ss, sp], lambda: mt.vjp(ss.buf, sp.buf, g), fetch)
    assert all(_bits(a) == _bits(b) for a, b in zip(got, base))
    got = run_on_stream(torch, S, form, [ss, sp], lambda: (mt(ss.buf, sp.buf),), fetch)
    assert _bits(got[0]) == _bits(base[0])

    # autograd under the stream (backward waits on the host for the engine's thread: no self-check)
    def autograd():
        ls, lp = ss.buf.clone().requires_grad_(), sp.buf.clone().requires_grad_()
        mt(ls, lp).backward(g)
        return (ls.grad, lp.grad)
    got = run_on_stream(torch, S, form, [ss, sp], autograd, fetch, returns_early=False)
    assert _bits(got[0]) == _bits(base[1]) and _bits(got[1]) == _bits(base[2])


# ---- 7. autograd and the renderer

def test_autograd_equals_vjp(psdr):
    import torch
    shape, sdf, pos = _case(seed=60)
    mt = psdr.MarchingTetrahedra(shape)
    topo = mt.extract(_t(sdf))
    V = topo.num_vertices
    g = _t(np.random.default_rng(62).uniform(-1, 1, (V, 3)).astype(np.float32)).cuda()
    v, gs, gp = mt.vjp(_t(sdf), _t(pos), g)
    assert v.shape == (V, 3) and v.dtype == torch.float32 and v.is_cuda and not v.requires_grad and not gs.requires_grad and gs.shape == (len(sdf),) and gp.shape == (len(sdf), 3)
    worst = {}
    r = ref.reference(sdf, pos, shape, _np(g))
    _held("autograd", worst, "v", _np(v), r["v32"], r["v64"])
    _held("autograd", worst, "grad_sdf", _np(gs), r["gs32"], r["gs64"])
    _held("autograd", worst, "grad_pos", _np(gp), r["gp32"], r["gp64"])
    _report("autograd", worst)
    ls, lp = _t(sdf).cuda().requires_grad_(), _t(pos).cuda().requires_grad_()
    out = mt(ls, lp)
    assert out.shape == (V, 3) and out.is_cuda and torch.equal(out.detach(), v)
    out.backward(g)
    assert torch.equal(ls.grad, gs) and torch.equal(lp.grad, gp)
    # float64 inputs on the host: the gradients return to their device and dtype
    hs, hp = _t(sdf.astype(np.float64)).requires_grad_(), _t(pos.astype(np.float64)).requires_grad_()
    mt(hs, hp).backward(g)
    assert hs.grad.dtype == torch.float64 and not hs.grad.is_cuda and torch.equal(hs.grad, gs.cpu().double())
    assert hp.grad.dtype == torch.float64 and not hp.grad.is_cuda and torch.equal(hp.grad, gp.cpu().double())
    # pos a constant: only sdf receives a gradient
    hs2 = _t(sdf).requires_grad_()
    mt(hs2, _t(pos)).backward(g)
    assert torch.equal(hs2.grad, gs.cpu())
    # a later extract does not disturb a graph made before it
    ls.grad = None
    out = mt(ls, lp)
    mt.extract(_t(np.roll(sdf, 5)))
    out.backward(g)
    assert torch.equal(ls.grad, gs)


def test_gradient_of_a_render_reaches_the_lattice(psdr):
    """a sphere extracted from a 9^3 lattice inside a Cornell-style box at 16 x 16 and 2 spp: sdf.grad is finite, non-zero on some ends of crossing edges and exactly zero
    on every lattice vertex that is no end of a crossing edge"""
    import torch
    from psdr_jit_amd import Matrix4fC, Matrix4fD
    D = scenes.DATA
    shape = (9, 9, 9)
    pos = psdr.lattice_points(shape, (158.0, 53.0, 160.0), (398.0, 293.0, 400.0))
    centre, radius = np.array([277.3, 171.9, 281.1]), 84.7
    sdf0 = (np.linalg.norm(pos.numpy().astype(np.float64) - centre, axis=1) - radius).astype(np.float32)
    assert np.abs(sdf0).min() >= 1e-2
    sdf = _t(sdf0).requires_grad_()
    mt = psdr.MarchingTetrahedra(shape)
    topo = mt.extract(sdf)
    r = ref.topology(sdf0, shape)
    _same_topology("ball", topo, r)
    assert ref.closed_and_oriented(_np(topo.faces))
    v = mt(sdf, pos)
    ball = mt.to_mesh(v)
    assert (int(ball.num_vertices), int(ball.num_faces)) == (topo.num_vertices, topo.num_faces)
    assert np.array_equal(np.asarray(ball.face_indices).reshape(-1, 3), _np(topo.faces))
    sc = psdr.Scene()
    sc.opts.spp, sc.opts.sppe, sc.opts.sppse = 2, 2, 2
    sc.opts.width = sc.opts.height = 16
    sc.opts.log_level = 0
    cam = psdr.PerspectiveCamera(60, 0.000001, 10000000.)
    cam.to_world = Matrix4fD([[1., 0., 0., 278.], [0., 1., 0., 273.], [0., 0., 1., -500.], [0., 0., 0., 1.]])
    sc.add_Sensor(cam)
    sc.add_BSDF(psdr.DiffuseBSDF([0.0, 0.0, 0.0]), "light")
    sc.add_BSDF(psdr.DiffuseBSDF([0.9, 0.6, 0.1]), "ball")
    sc.add_BSDF(psdr.DiffuseBSDF([0.95, 0.95, 0.95]), "white")
    I = np.eye(4, dtype=np.float32).tolist()
    sc.add_Mesh(os.path.join(D, "cbox_luminaire.obj"), Matrix4fC([[1., 0., 0., 0.], [0., 1., 0., -0.5], [0., 0., 1., 0.], [0., 0., 0., 1.]]), "light", psdr.AreaLight([20.0, 20.0, 8.0]))
    sc.add_Mesh(ball, "ball", None)
    for f in ("cbox_floor", "cbox_back"):
        sc.add_Mesh(os.path.join(D, f + ".obj"), Matrix4fC(I), "white", None)
    sc.configure()
    sc.configure([0])
    img = psdr.PathTracer(2).renderD(sc, 0, seed=9)
    img.sum().backward()
    assert sdf.grad is not None and tuple(sdf.grad.shape) == (len(sdf0),) and not sdf.grad.is_cuda
    grad = sdf.grad.numpy()
    ends = np.zeros(len(sdf0), bool)
    ends[r["edges"].ravel()] = True
    assert np.isfinite(grad).all() and (grad[ends] != 0).any() and not grad[~ends].any()
    print("sdf.grad: %d of %d ends of crossing edges are non-zero, max |grad| = %.3g" % ((grad[ends] != 0).sum(), ends.sum(), np.abs(grad).max()))
