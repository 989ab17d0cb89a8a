"""GPU tests of the point-to-mesh distance (psdr_jit_amd/pointmesh.py, csrc/hip/pointmesh.hip) against the numpy checker tests/pointmesh_ref.py.

Face indices are not compared for equality: on a closed mesh a point nearest a shared edge or vertex is equally near several faces, and float32 and float64 pick
differently (tests/pointmesh_ref.py).  What is compared is unique, per case and per array by the rule of tests/test_gpu_meshreg.py, e_gpu <= 4 max(e_32, u G), u = 2^-24:
    dist2_p, dist2_f          against the float64 minima
    q_p, q_f                  the closest points bary . v[faces[face]], against float64's
    chosen_p, chosen_f        the float64 dist2 of the pair the device chose, against the float64 minimum
    loss, terms, d / dpoints, d / dv      against the float64 evaluation THROUGH THE DEVICE'S INDICES
with e_32 the same deviation of the float32 checker (its own indices, its own barycentrics).  Also: every bary in [0, 1] and every row summing to 1 within 4 u, every
index in range, dist2 >= 0.  Every test prints the worst ratio it saw per array.

Measured on an MI355X, the worst e_gpu / max(e_32, u G) over all cases: dist2_p, dist2_f, q_p, q_f, the chosen pair of a point and both gradients
1.00 (the float32 checker's own error: the device has its operation order), the chosen pair of a face 0.00, values 1.45 (F = 1).  The shape recovery fell from 1.56e-3 to
2.34e-4, a ratio of 0.15.

Then the exact cases (points on vertices, dyadic interior points, the tie rule in both directions), weights, repeatability, both stream forms of tests/stream_cases.py,
autograd through Subdivision and the Laplacian preconditioner, and a shape recovery."""
import numpy as np
import pytest

import chamfer_ref as cref
import pointmesh_ref as ref
from stream_cases import Slot, run_on_stream, run_plain

pytestmark = pytest.mark.gpu

NS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1026, 2049)
CONFIGS = (("point -> face", (1.0, 0.0)), ("face -> point", (0.0, 1.0)), ("both", (1.0, 0.5)))


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


def _call(pm, p, v):
    """-> (loss, terms [2], d / dpoints, d / dv, nearest as numpy or None) of one value_and_grad"""
    loss, gp, gv = pm.value_and_grad(_t(p), _t(v))
    near = tuple(None if a is None else a.cpu().numpy() for a in pm.nearest)
    return float(loss.cpu()), pm.terms.cpu().numpy(), gp.cpu().numpy(), gv.cpu().numpy(), near


def _held(what, worst, key, dev, f32, f64):
    r, e_gpu, e_32, G = ref.ratio(dev, f32, f64)
    worst[key] = max(worst.get(key, 0.0), r)
    assert np.isfinite(np.asarray(dev)).all(), what
    assert r <= 4.0, "%s, %s: e_gpu = %.3g, e_32 = %.3g, u G = %.3g: ratio %.3g > 4" % (what, key, e_gpu, e_32, ref.U * G, r)


def _q(v, f, face, bary):
    """bary . v[faces[face]] in float64"""
    c = np.asarray(v, np.float64)[np.asarray(f, np.int64)[np.asarray(face, np.int64)]]
    return (np.asarray(bary, np.float64)[:, :, None] * c).sum(1)


def _sane(what, index, bary, dist2, count):
    assert index.dtype == np.int32 and bary.dtype == np.float32 and dist2.dtype == np.float32, what
    assert (index >= 0).all() and (index < count).all(), what
    assert np.isfinite(bary).all() and np.isfinite(dist2).all() and (dist2 >= 0).all(), what
    assert bary.min() >= -4 * ref.U and bary.max() <= 1 + 4 * ref.U, (what, bary.min(), bary.max())
    assert np.abs(bary.astype(np.float64).sum(1) - 1.0).max() <= 4 * ref.U, what


def _nearest_held(what, worst, p, v, f, near, c64, c32, directions=(0, 1)):
    """the three arrays of each direction under the rule"""
    N, F = len(p), len(f)
    if 0 in directions:
        a, bary, d = near[0], near[1], near[2]
        assert a.shape == (N,) and bary.shape == (N, 3) and d.shape == (N,)
        _sane(what, a, bary, d, F)
        _held(what, worst, "dist2_p", d, c32.dist2_p, c64.dist2_p)
        _held(what, worst, "q_p", _q(v, f, a, bary), _q(v, f, c32.face_of_point, c32.bary_p), _q(v, f, c64.face_of_point, c64.bary_p))
        at = np.arange(N)
        _held(what, worst, "chosen_p", ref.chosen(p, v, f, at, a)[1], ref.chosen(p, v, f, at, c32.face_of_point)[1], c64.dist2_p)
    if 1 in directions:
        b, bary, d = near[3], near[4], near[5]
        assert b.shape == (F,) and bary.shape == (F, 3) and d.shape == (F,)
        _sane(what, b, bary, d, N)
        at = np.arange(F)
        _held(what, worst, "dist2_f", d, c32.dist2_f, c64.dist2_f)
        _held(what, worst, "q_f", _q(v, f, at, bary), _q(v, f, at, c32.bary_f), _q(v, f, at, c64.bary_f))
        _held(what, worst, "chosen_f", ref.chosen(p, v, f, b, at)[1], ref.chosen(p, v, f, c32.point_of_face, at)[1], c64.dist2_f)


def _values_held(what, worst, p, v, f, w, squared, out, near):
    """loss, terms and both gradients against the float64 evaluation through the device's indices"""
    loss, terms, gp, gv = out
    f64 = ref.evaluate(p, v, f, near[0], near[3], w, squared, np.float64)
    f32 = ref.evaluate(p, v, f, near[0], near[3], w, squared, np.float32)
    for k in range(2):
        if w[k] > 0:
            _held(what, worst, "value", terms[k], f32["terms"][k], f64["terms"][k])
        else:
            assert terms[k] == 0 and near[3 * k] is None and near[3 * k + 1] is None and near[3 * k + 2] is None
    _held(what, worst, "value", loss, f32["loss"], f64["loss"])
    _held(what, worst, "d/dpoints", gp, f32["gp"], f64["gp"])
    _held(what, worst, "d/dv", gv, f32["gv"], f64["gv"])


def _report(what, worst):
    print("%s: worst e_gpu / max(e_32, u G): %s" % (what, ", ".join("%s %.2f" % kv for kv in sorted(worst.items()))))


# ---- the plan's boundaries

@pytest.mark.parametrize("which", range(5))
def test_sizes_on_the_edges_of_the_plan(psdr, which):
    """every N on the wave's, the workgroup's and the queries-per-lane edges against F in {1, tile - 1, tile, tile + 1, 2 tile + 1}, tile read from the plan: N = 1 with
    F = 2 tile + 1 is one point against three slices, F = 1 is one face against N points.  One lattice and one cloud; every (N, F) is a leading block of them"""
    plan = psdr.launch_plan_pm
    tile = plan(1, 1).tile
    fs = (1, tile - 1, tile, tile + 1, 2 * tile + 1)
    F = fs[which]
    assert len({plan(n, 1).queries_per_lane for n in NS}) >= 2 and plan(1, fs[-1]).slices >= 3 and plan(fs[-1], 1).queries_per_lane >= 1
    p_all, v, f_all, d64, d32 = ref.sweep_reference(max(NS), fs[-1])
    f = f_all[:F]
    pm = psdr.PointMeshDistance(f, len(v), weights=(1.0, 0.5))
    worst = {}
    for N in NS:
        p = p_all[:N]
        c64 = ref.closest_from_matrix(p, v, f, d64[:N, :F], np.float64)
        c32 = ref.closest_from_matrix(p, v, f, d32[:N, :F], np.float32)
        loss, terms, gp, gv, near = _call(pm, p, v)
        what = "N = %d, F = %d, plans %s / %s" % (N, F, tuple(plan(N, F)), tuple(plan(F, N)))
        _nearest_held(what, worst, p, v, f, near, c64, c32)
        _values_held(what, worst, p, v, f, pm.weights, True, (loss, terms, gp, gv), near)
    _report("F = %d" % F, worst)


# ---- the named cases

@pytest.mark.parametrize("squared", [True, False])
@pytest.mark.parametrize("name", ref.CASES)
def test_accuracy_rule(psdr, name, squared):
    """regions (every region of the cascade wins for many points), near (the winners are interior), degenerate (a zero-area face, a zero-length edge, a sliver): each
    direction alone and both with the weights (1, 0.5)"""
    p, v, f, c64, c32 = ref.reference(name)
    pm = psdr.PointMeshDistance(f, len(v), squared=squared)
    worst = {}
    for label, w in CONFIGS:
        pm.weights = w
        loss, terms, gp, gv, near = _call(pm, p, v)
        what = "%s, squared = %s, %s" % (name, squared, label)
        _nearest_held(what, worst, p, v, f, near, c64, c32, [k for k in (0, 1) if w[k] > 0])
        _values_held(what, worst, p, v, f, w, squared, (loss, terms, gp, gv), near)
        assert np.isfinite(gp).all() and np.isfinite(gv).all()          # (the degenerate faces receive no NaN)
    if name == "degenerate":
        assert {6, 7, 8} <= set(c64.face_of_point.tolist())          # (the case reaches the three degenerate faces)
    _report("%s, squared = %s" % (name, squared), worst)


def test_closest_points_on_mesh(psdr):
    """the function form: the same three arrays as pm.nearest's first direction, bit for bit, detached, on the device"""
    import torch
    p, v, f, c64, c32 = ref.reference("near")
    face, bary, d2 = psdr.closest_points_on_mesh(_t(p), _t(v), f)
    assert face.dtype == torch.int32 and bary.dtype == d2.dtype == torch.float32 and face.is_cuda and bary.is_cuda and d2.is_cuda and not bary.requires_grad
    near = (face.cpu().numpy(), bary.cpu().numpy(), d2.cpu().numpy())
    worst = {}
    _nearest_held("closest_points_on_mesh", worst, p, v, f, near, c64, c32, (0,))
    pm = psdr.PointMeshDistance(f, len(v), weights=(1.0, 0.0))
    pm.value_and_grad(_t(p), _t(v))
    assert all(_bits(a) == _bits(b.cpu().numpy()) for a, b in zip(near, pm.nearest[:3]))
    again = psdr.closest_points_on_mesh(_t(p).double(), _t(v).cuda(), _t(f.astype(np.int32)).cuda())          # other dtypes and devices, faces already on the GPU
    assert all(_bits(a) == _bits(b.cpu().numpy()) for a, b in zip(near, again))
    _report("closest_points_on_mesh", worst)


# ---- exact cases

@pytest.mark.parametrize("squared", [True, False])
def test_points_on_the_vertices(psdr, squared):
    """the points are the mesh's own vertices: every dist2 is exactly 0 and all gradients are exactly 0 in both modes - rho' at 0 is defined as 0"""
    v, f = ref.bunny()
    pm = psdr.PointMeshDistance(f, len(v), squared=squared)
    for _label, w in CONFIGS:
        pm.weights = w
        loss, terms, gp, gv, near = _call(pm, v[np.unique(f)], v)          # (the vertices a face names)
        assert loss == 0 and not terms.any() and not gp.any() and not gv.any() and np.isfinite(gp).all() and np.isfinite(gv).all()
        for k in (2, 5):
            assert near[k] is None or not near[k].any()


def _dyadic():
    """a lattice whose coordinates are multiples of 1 / 4, and per face five points with dyadic barycentrics: every product of the pair function is exact"""
    k = 4
    idx = lambda i, j: i * (k + 1) + j
    v = np.array([[i / 4.0, j / 4.0, ((i * j + i) % 3) / 4.0] for i in range(k + 1) for j in range(k + 1)], np.float64)
    faces = []
    for i in range(k):
        for j in range(k):
            faces += [(idx(i, j), idx(i + 1, j), idx(i, j + 1)), (idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1))]
    f = np.array(faces, np.int64)
    st = np.array([[0.25, 0.25], [0.5, 0.25], [0.125, 0.625], [0.375, 0.5], [0.0625, 0.0625]])
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    p = a[:, None, :] + st[None, :, 0:1] * (b - a)[:, None, :] + st[None, :, 1:2] * (c - a)[:, None, :]
    owner = np.repeat(np.arange(len(f)), len(st))
    bary = np.tile(np.stack([1 - st.sum(1), st[:, 0], st[:, 1]], 1), (len(f), 1))
    p32 = p.reshape(-1, 3).astype(np.float32)
    assert np.array_equal(p32.astype(np.float64), p.reshape(-1, 3))
    return p32, v.astype(np.float32), f, owner, bary.astype(np.float32)


def test_points_in_the_interior_with_dyadic_barycentrics(psdr):
    """dist2 is exactly 0, the face is the point's own (it is interior: no other face holds it) and the barycentrics are the exact ones"""
    p, v, f, owner, bary = _dyadic()
    pm = psdr.PointMeshDistance(f, len(v))
    loss, terms, gp, gv, near = _call(pm, p, v)
    assert not near[2].any() and not near[5].any() and loss == 0 and not gp.any() and not gv.any()
    assert np.array_equal(near[0], owner) and _bits(near[1]) == _bits(bary)
    assert (owner[near[3]] == np.arange(len(f))).all()          # every face's nearest point is one of its own five


# ---- the tie rule

def _tie_placements(plan, queries, base_count):
    """(count, at, copy_at, where): the copy in the same tile, in another tile of the same slice, in another slice, and in the last slice as the last candidate of a
    partial tile with the winner as candidate 0"""
    p = plan(queries, base_count)
    count = base_count
    assert count % p.tile != 0 and p.slices >= 3
    at = 5
    out = [(count, at, at + 2, "the same tile"), (count, at, at + p.slice_len, "another slice"), (count, 0, count - 1, "the last slice")]
    if p.slice_len >= 2 * p.tile:
        out.insert(1, (count, at, at + p.tile, "another tile"))
    for _c, a, c, where in out:
        assert (a // p.tile == c // p.tile) == (where == "the same tile") and (a // p.slice_len == c // p.slice_len) == (where in ("the same tile", "another tile"))
    return out


def _long_count(plan, queries):
    """a candidate count at which a slice of `queries` queries holds two tiles, ending in a partial tile one candidate into a slice"""
    m = cref.first_long_slice(plan, queries)
    length = plan(queries, m).slice_len
    return length * (-(-m // length) + 1) + 1


def test_the_lower_face_wins_a_tie(psdr):
    """an exact copy of the winning face (the same three vertex ids) at a higher index: the device reports the lower index each time, for one point (slices of two tiles)
    and for 300 points (one tile per slice).  Identical inputs give identical bits: no tolerance"""
    plan = psdr.launch_plan_pm
    tile = plan(1, 1).tile
    seen = set()
    for N, F in ((1, _long_count(plan, 1)), (300, 4 * tile + 9)):
        v0, f0 = ref.lattice(F)
        v0 = v0 + np.float32([5.0, 0.0, 0.0])                                    # every other face is far away
        tri = np.float32([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.0, 0.5, 0.1]])
        v = np.concatenate([v0, tri])
        ids = len(v0) + np.arange(3)
        p = (np.float32([0.15, 0.15, 0.1]) + np.float32(0.05) * cref._uniform(N, 51)).astype(np.float32)
        for count, at, copy_at, where in _tie_placements(plan, N, F):
            f = f0.copy()
            f[at] = f[copy_at] = ids
            face, bary, d2 = (a.cpu().numpy() for a in psdr.closest_points_on_mesh(_t(p), _t(v), f))
            assert (face == at).all(), "N = %d, F = %d, a copy in %s: face %s, not %d" % (N, F, where, np.unique(face), at)
            want = ref.chosen(p, v, f, np.arange(N), np.full(N, at), np.float32)
            assert _bits(d2) == _bits(want[1]) and _bits(bary) == _bits(want[0])          # (and the winner's numbers are the checker's, bit for bit)
            seen.add(where)
    assert seen == {"the same tile", "another tile", "another slice", "the last slice"}


def test_the_lower_point_wins_a_tie(psdr):
    """the second direction: a duplicated point at a higher index, for one face and for 300 faces"""
    plan = psdr.launch_plan_pm
    tile = plan(1, 1).tile
    seen = set()
    for F, N in ((1, _long_count(plan, 1)), (300, 4 * tile + 9)):
        v, f = ref.lattice(F)
        pm = psdr.PointMeshDistance(f, len(v), weights=(0.0, 1.0))
        base = cref._uniform(N, 52, 4.0, 5.0)                                     # every other point is far away
        near_point = np.float32([0.4, 0.45, 0.3])
        for count, at, copy_at, where in _tie_placements(plan, F, N):
            p = base.copy()
            p[at] = p[copy_at] = near_point
            _loss, _terms, _gp, _gv, near = _call(pm, p, v)
            assert (near[3] == at).all(), "F = %d, N = %d, a copy in %s: point %s, not %d" % (F, N, where, np.unique(near[3]), at)
            want = ref.chosen(p, v, f, np.full(F, at), np.arange(F), np.float32)
            assert _bits(near[5]) == _bits(want[1]) and _bits(near[4]) == _bits(want[0])
            seen.add(where)
    assert seen == {"the same tile", "another tile", "another slice", "the last slice"}


# ---- weights, repeatability

@pytest.mark.parametrize("squared", [True, False])
def test_a_direction_of_weight_zero_is_left_out(psdr, squared):
    """its value is exactly 0 and its arrays are None; the other direction's gradients keep their bits: the point gradient with both on is the float32 sum of the two
    single-direction gradients (each point adds the two once), and a second object that never had the other weight gives the same bits"""
    p, v, f, _c64, _c32 = ref.reference("near")
    pm = psdr.PointMeshDistance(f, len(v), squared=squared)
    w = (0.75, 1.5)
    pm.weights = (w[0], 0.0)
    a = _call(pm, p, v)
    pm.weights = (0.0, w[1])
    b = _call(pm, p, v)
    assert a[1][1] == 0 and b[1][0] == 0 and a[1][0] > 0 and b[1][1] > 0 and a[0] == np.float32(w[0]) * a[1][0] and b[0] == np.float32(w[1]) * b[1][1]
    assert all(x is None for x in a[4][3:]) and all(x is None for x in b[4][:3])
    assert all(np.abs(x).max() > 0 for x in (a[2], a[3], b[2], b[3]))
    pm.weights = w
    both = _call(pm, p, v)
    assert both[1][0] == a[1][0] and both[1][1] == b[1][1] and np.float32(both[0]) == np.float32(a[0]) + np.float32(b[0])
    assert _bits(both[2]) == _bits(a[2] + b[2]) and both[2].dtype == np.float32
    for k in range(3):
        assert _bits(both[4][k]) == _bits(a[4][k]) and _bits(both[4][3 + k]) == _bits(b[4][3 + k])
    for weights, one in (((w[0], 0.0), a), ((0.0, w[1]), b)):
        again = _call(psdr.PointMeshDistance(f, len(v), weights=weights, squared=squared), p, v)
        assert again[0] == one[0] and _bits(again[2]) == _bits(one[2]) and _bits(again[3]) == _bits(one[3])
    pm.weights = (0.0, 0.0)
    loss, terms, gp, gv, near = _call(pm, p, v)
    assert loss == 0 and not terms.any() and not gp.any() and not gv.any() and all(x is None for x in near)


def test_ten_calls_return_identical_bits(psdr):
    """the loss, the terms, both gradients, the indices, the barycentrics and the distances; both scans in several slices"""
    import torch
    p, v, f, _c64, _c32 = ref.reference("regions")
    assert psdr.launch_plan_pm(len(p), len(f)).slices >= 3 and psdr.launch_plan_pm(len(f), len(p)).slices >= 3
    pd, vd = _t(p).cuda(), _t(v).cuda()
    pm = psdr.PointMeshDistance(f, len(v), weights=(1.0, 0.5), squared=False)
    runs = []
    for _ in range(10):
        loss, gp, gv = pm.value_and_grad(pd, vd)
        runs.append(tuple(_bits(t.cpu().numpy()) for t in (loss, pm.terms, gp, gv) + tuple(pm.nearest)))
    assert all(r == runs[0] for r in runs[1:])
    fd = _t(f.astype(np.int32)).cuda()
    first = tuple(_bits(t.cpu().numpy()) for t in psdr.closest_points_on_mesh(pd, vd, fd))
    assert all(tuple(_bits(t.cpu().numpy()) for t in psdr.closest_points_on_mesh(pd, vd, fd)) == first for _ in range(9))
    assert torch.cuda.is_available()


# ---- streams

@pytest.mark.parametrize("form", ("S", "default"))
def test_streams(psdr, form):
    """both forms of the delayed producer on pm(points, v) plus its backward and on closest_points_on_mesh: points and v rolled along their first axis are the decoys"""
    import torch
    import stream_cases as sc_
    p, v, f, _c64, _c32 = ref.reference("near")
    pm = psdr.PointMeshDistance(f, len(v), weights=(1.0, 0.5))
    sp, sv = Slot(torch, p), Slot(torch, v)
    fd = _t(f.astype(np.int32)).cuda()
    fetch = lambda t: tuple(a.cpu().numpy() for a in t)
    call = lambda: pm.value_and_grad(sp.buf, sv.buf) + (pm.terms,) + tuple(pm.nearest)
    base = run_plain(torch, [sp, sv], call, fetch)
    for k, (dp_, dv_) in enumerate(((sc_.decoy_of(p), v), (p, sc_.decoy_of(v)))):          # (each decoy is told apart)
        decoy = _call(pm, dp_, dv_)
        assert _bits(decoy[2 + k]) != _bits(base[1 + k])
    S = torch.cuda.Stream()

    # autograd under the stream first (backward waits on the host for the engine's thread: no self-check)
    def autograd():
        lp, lv = sp.buf.clone().requires_grad_(), sv.buf.clone().requires_grad_()
        pm(lp, lv).backward()
        return (lp.grad, lv.grad)
    got = run_on_stream(torch, S, form, [sp, sv], autograd, fetch, returns_early=False)
    assert _bits(got[0]) == _bits(base[1]) and _bits(got[1]) == _bits(base[2])
    # the Python layer returns without a synchronisation: the delay is still running when it does
    got = run_on_stream(torch, S, form, [sp, sv], call, fetch)
    assert all(_bits(a) == _bits(b) for a, b in zip(got, base))
    got = run_on_stream(torch, S, form, [sp, sv], lambda: psdr.closest_points_on_mesh(sp.buf, sv.buf, fd), fetch)
    assert all(_bits(got[k]) == _bits(base[4 + k]) for k in range(3))


# ---- autograd

def test_autograd_scales_the_forward_gradients(psdr):
    import torch
    p, v, f, _c64, _c32 = ref.reference("near")
    pm = psdr.PointMeshDistance(f, len(v), weights=(1.0, 0.5))
    loss, gp, gv = pm.value_and_grad(_t(p), _t(v))
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda and not loss.requires_grad and not gp.requires_grad and pm.terms.shape == (2,)
    assert gp.shape == (len(p), 3) and gv.shape == (len(v), 3)
    lp, lv = _t(p).cuda().requires_grad_(), _t(v).cuda().requires_grad_()
    out = pm(lp, lv)
    assert out.dim() == 0 and out.dtype == torch.float32 and out.is_cuda and out.item() == loss.item() and not pm.terms.requires_grad
    (3 * out).backward()
    assert torch.equal(lp.grad, 3 * gp) and torch.equal(lv.grad, 3 * gv)
    # v on the host in float64, the points a constant: the gradient returns to v's device and dtype
    hv = _t(v.astype(np.float64)).requires_grad_()
    (3 * pm(_t(p), hv)).backward()
    assert hv.grad.dtype == torch.float64 and not hv.grad.is_cuda and torch.equal(hv.grad, (3 * gv).cpu().double())
    # the plain attributes are read at every call
    pm.weights, pm.squared = (0.0, 1.0), False
    assert pm(lp, lv).item() == pm.terms[1].item() and pm.terms[0].item() == 0
    pm.weights = (1.0, -1.0)
    with pytest.raises(ValueError):
        pm(lp, lv)


def test_autograd_through_subdivision_and_the_preconditioner(psdr):
    """pm(points, sub.refine(c)).backward() and pm(points, pre.from_differential(u)).backward() reach c and u; the vertex gradient that enters them is value_and_grad's,
    bit for bit"""
    import torch
    import meshreg_ref
    faces, n, c0 = meshreg_ref.case("grid9")
    sub = psdr.Subdivision(np.array(faces), n, levels=1)
    fine = sub.refine(_t(c0)).cpu().numpy()
    points = _t((fine[::2] + np.float32([0.02, -0.03, 0.15])).astype(np.float32)).cuda()
    pm = psdr.PointMeshDistance(sub.faces, sub.num_vertices_out)
    c = _t(c0).cuda().requires_grad_()
    pm(points, sub.refine(c)).backward()
    _loss, _gp, gv = pm.value_and_grad(points, sub.refine(c.detach()))
    assert gv.abs().max() > 0 and torch.equal(c.grad, sub.restrict(gv))
    leaf = sub.refine(c.detach()).requires_grad_()
    pm(points, leaf).backward()
    assert torch.equal(leaf.grad, gv)
    pre = psdr.LaplacianPreconditioner(np.array(faces), n)
    coarse = psdr.PointMeshDistance(np.array(faces), n)
    pts = _t((c0 + np.float32([0.02, -0.03, 0.15])).astype(np.float32)).cuda()
    u = pre.to_differential(_t(c0)).detach().requires_grad_()
    coarse(pts, pre.from_differential(u)).backward()
    _loss, _gp, g = coarse.value_and_grad(pts, pre.from_differential(u.detach()))
    want = pre.from_differential(g)
    assert g.norm() > 0 and (u.grad - want).norm().item() <= 2 * pre.rtol * g.norm().item()


def test_shape_recovery(psdr):
    """the bunny's vertices displaced by the smooth offset of 5 % of the bounding box of tests/test_gpu_chamfer.py, 5 000 points drawn ONCE from the target surface, 50
    steps of AdamUniform on pm(points, v), both directions: the loss ends below half of its start.  No resample and no read-back inside the loop"""
    import torch
    V, f = ref.bunny()
    box = float((V.max(0) - V.min(0)).max())
    offset = 0.05 * box * np.stack([np.sin(3.0 * V[:, 1] + 1.0), np.sin(3.0 * V[:, 2] + 2.0), np.cos(3.0 * V[:, 0])], 1)
    assert 0.03 * box <= np.linalg.norm(offset, axis=1).max() <= 0.05 * box * np.sqrt(3.0)
    points = psdr.SurfaceSampler(f, len(V), num_points=5000, seed=5).resample(V)(_t(V)).detach()
    v = _t((V + offset).astype(np.float32)).cuda().requires_grad_()
    pm = psdr.PointMeshDistance(f, len(V))
    opt = psdr.AdamUniform([v], lr=0.002)
    losses = []
    for _step in range(50):
        opt.zero_grad()
        loss = pm(points, v)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    start, end = losses[0].item(), pm(points, v.detach()).item()
    print("shape recovery: point-to-mesh loss %.4g -> %.4g (ratio %.3f)" % (start, end, end / start))
    assert np.isfinite(end) and end < 0.5 * start, "the loss fell from %.4g to %.4g only" % (start, end)
