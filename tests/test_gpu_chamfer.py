"""GPU tests of the Chamfer distance and the surface sampler (psdr_jit_amd/chamfer.py, csrc/hip/chamfer.hip) against the numpy checker tests/chamfer_ref.py.

Indices and distances: nearest_points equals the checker's float32 scan bit for bit - both arrays, no tolerance - on sizes read from launch_plan (N on the wave's and the
workgroup's edges and where the plan changes the queries per lane; M on the tile's and the slices' edges) and on the named cases: one query against all slices, many
queries against one candidate, the nearest as the last candidate of the last partial tile and as candidate 0, exact duplicates of the winner in the same tile, in another
tile and in another slice, all of y identical, x identical to y, a lattice of exact ties, clouds around 1000 with a spacing of 1e-3 (where the expansion form fails), the
bunny against a jittered copy.

Value and gradient: the rule of tests/test_gpu_meshreg.py, e_gpu <= 4 max(e_32, u G) with u = 2^-24, per direction and for the sum, for both settings of `squared`,
against the float64 evaluation through the same, bit-defined, indices.  Every test prints the worst ratio it saw.

Measured on an MI355X, the worst e_gpu / max(e_32, u G) over all cases: values - x -> y alone 0.65 (wide), y -> x alone 0.80 (one_candidate, Euclidean),
both directions 1.34 (identical_y, squared); gradients 1.00 everywhere (the float32 checker's own error).  The shape recovery fell from 1.83e-3 to 3.9e-4, a ratio of 0.21.

Then the exact cases (x == y, a direction of weight 0, a hub of 300 members), repeatability, both stream forms of tests/stream_cases.py, autograd through the sampler,
Subdivision and the Laplacian preconditioner, and a shape recovery."""
import numpy as np
import pytest

import chamfer_ref as ref
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


def _nearest(psdr, x, y):
    import torch
    idx, d2 = psdr.nearest_points(torch.from_numpy(np.ascontiguousarray(x)), torch.from_numpy(np.ascontiguousarray(y)))
    assert idx.dtype == torch.int32 and d2.dtype == torch.float32 and idx.is_cuda and d2.is_cuda and not idx.requires_grad and not d2.requires_grad
    return idx.cpu().numpy(), d2.cpu().numpy()


def _same(psdr, x, y, what, want=None):
    idx, d2 = _nearest(psdr, x, y)
    want = ref.nearest(x, y) if want is None else want
    assert idx.shape == want[0].shape and d2.shape == want[1].shape
    bad = np.nonzero((idx != want[0]) | (d2.view(np.uint32) != want[1].view(np.uint32)))[0]
    assert bad.size == 0, "%s: %d of %d differ, first at %d: device (%d, %r), checker (%d, %r)" % (what, bad.size, len(idx), bad[0], idx[bad[0]], d2[bad[0]], want[0][bad[0]], want[1][bad[0]])


def test_sizes_on_the_edges_of_the_plan(psdr):
    """every N on the plan's edges against every M on them, both arrays bit for bit"""
    plan = psdr.launch_plan
    ns, ms = ref.query_sizes(plan), ref.candidate_sizes(plan)
    tile = plan(1, 1).tile
    assert {1, 63, 64, 65} <= set(ns) and {1, tile - 1, tile, tile + 1} <= set(ms)
    assert len({plan(n, 1).queries_per_lane for n in ns}) >= 2                      # (both scans are reached)
    assert max(plan(ns[0], m).slices for m in ms) >= 3                               # (a size with at least three slices)
    xs, ys = ref._uniform(max(ns), 21), ref._uniform(max(ms), 22)
    for m in ms:
        for n in ns:
            _same(psdr, xs[:n], ys[:m], "N = %d, M = %d, plan %s" % (n, m, tuple(plan(n, m))))


def test_slices_longer_than_a_tile(psdr):
    """N = 1 and M large: all slices and one query; M = slice_len k +- 1 and slice_len k, with slice_len read from the plan and above one tile"""
    plan = psdr.launch_plan
    x, y, ia, da, _ib, _db = ref.reference("one_query", plan)
    m = len(y)
    p = plan(1, m)
    assert p.slice_len > p.tile and p.slices >= 3 and (m - 1) % p.slice_len == 0
    _same(psdr, x, y, "one query, M = %d" % m, (ia, da))
    for cut in (m - 1, m - 2):
        assert plan(1, cut).slice_len == p.slice_len
        _same(psdr, x, y[:cut], "one query, M = %d" % cut)
    x3 = ref._uniform(3, 23)
    _same(psdr, x3, y, "three queries, M = %d" % m)


@pytest.mark.parametrize("name", [c for c in ref.CASES if c != "one_query"])
def test_named_cases_bit_for_bit(psdr, name):
    """both directions of every named case"""
    plan = psdr.launch_plan
    x, y, ia, da, ib, db = ref.reference(name, plan)
    _same(psdr, x, y, name + ", x -> y", (ia, da))
    _same(psdr, y, x, name + ", y -> x", (ib, db))
    if name == "last":
        assert (ia == len(y) - 1).all() and len(y) % plan(len(x), len(y)).tile != 0
    if name == "first":
        assert (ia == 0).all()
    if name == "identical_y":
        assert (ia == 0).all() and plan(len(x), len(y)).slices >= 3
    if name == "same":
        assert np.array_equal(ia, np.arange(len(x))) and not da.any()
    if name == "lattice":
        assert (da == 0).sum() > 100                                                # (many exact ties: a lattice point is hit several times)
    if name == "far":
        assert (ref.nearest_expansion(x, y) != ia).any()                            # (the expansion form fails here: the case pins the difference form)
    if name == "one_candidate":
        assert len(y) == 1 and plan(len(x), 1).queries_per_lane > 1
    if name == "hub":
        assert (ib[:300] == 0).all()


def test_exact_duplicates_of_the_winner(psdr):
    """an exact copy of the winner at a higher index - in the same tile, in another tile of the same slice, in another slice: the lower index wins each time, for a few
    queries (slices longer than a tile) and for many (one tile per slice)"""
    plan = psdr.launch_plan
    xq, y0, _ia, _da, _ib, _db = ref.reference("one_query", plan)
    p = plan(1, len(y0))
    assert p.slice_len >= 2 * p.tile
    at = 5
    for n, y_base, length in ((1, y0, p.slice_len), (300, ref._uniform(4 * p.tile + 9, 24, 2.0, 3.0), plan(300, 4 * p.tile + 9).slice_len)):
        x = (np.float32(0.25) + np.float32(0.01) * ref._uniform(n, 25)).astype(np.float32)
        for copy_at, where in ((at + 2, "the same tile"), (at + p.tile, "another tile"), (at + length, "another slice"), (len(y_base) - 1, "the last slice")):
            y = y_base.copy()
            y[:, 0] += np.float32(3.0)                                              # every other candidate is far away
            y[at] = y[copy_at] = np.float32(0.25)
            if n == 1:
                assert (at // p.tile == copy_at // p.tile) == (where == "the same tile") and (at // length == copy_at // length) == (where in ("the same tile", "another tile"))
            idx, d2 = _nearest(psdr, x, y)
            assert (idx == at).all(), "N = %d, a copy in %s: index %s" % (n, where, np.unique(idx))
            _same(psdr, x, y, "N = %d, a copy in %s" % (n, where))


# ---- value and gradient

CONFIGS = (("x -> y", (1.0, 0.0)), ("y -> x", (0.0, 1.0)), ("sum", (1.0, 0.5)))


def _call(cd, x, y):
    """-> (loss, terms [2], gx, gy) as numpy"""
    import torch
    loss, gx, gy = cd.value_and_grad(torch.from_numpy(np.ascontiguousarray(x)), torch.from_numpy(np.ascontiguousarray(y)))
    return float(loss.cpu()), cd.terms.cpu().numpy(), gx.cpu().numpy(), gy.cpu().numpy()


def _held(what, worst, key, dev, f32, f64):
    r, e_gpu, e_32, G = ref.ratio(dev, f32, f64)
    worst[key] = max(worst.get(key, 0.0), r)
    assert np.isfinite(np.asarray(dev)).all(), what
    assert r <= 4.0, "%s: e_gpu = %.3g, e_32 = %.3g, u G = %.3g: ratio %.3g > 4" % (what, e_gpu, e_32, ref.U * G, r)


@pytest.mark.parametrize("squared", [True, False])
@pytest.mark.parametrize("name", ref.CASES)
def test_accuracy_rule(psdr, name, squared):
    x, y, ia, _da, ib, _db = ref.reference(name, psdr.launch_plan)
    cd = psdr.ChamferDistance(squared=squared)
    worst = {}
    for label, w in CONFIGS:
        cd.weights = w
        loss, terms, gx, gy = _call(cd, x, y)
        near = cd.nearest
        for k, want in ((0, ia), (2, ib)):                                          # the device's indices are the checker's: the error is taken through the same indices
            if w[k // 2] > 0:
                assert np.array_equal(near[k].cpu().numpy(), want)
            else:
                assert near[k] is None and near[k + 1] is None
        f64 = ref.evaluate(x, y, ia, ib, w, squared, np.float64)
        f32 = ref.evaluate(x, y, ia, ib, w, squared, np.float32)
        what = "%s, squared = %s, %s" % (name, squared, label)
        for k in range(2):
            if w[k] > 0:
                _held(what + ": term %d" % k, worst, label + " value", terms[k], f32["terms"][k], f64["terms"][k])
            else:
                assert terms[k] == 0
        _held(what + ": loss", worst, label + " value", loss, f32["loss"], f64["loss"])
        _held(what + ": dx", worst, label + " dx", gx, f32["gx"], f64["gx"])
        _held(what + ": dy", worst, label + " dy", gy, f32["gy"], f64["gy"])
    print("%s, squared = %s: worst e_gpu / max(e_32, u G): %s" % (name, squared, ", ".join("%s %.2f" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("squared", [True, False])
def test_identical_sets_give_exactly_zero(psdr, squared):
    """x == y: the loss is exactly 0 and both gradients are exactly 0 in both modes - rho' at 0 is defined as 0"""
    x, y, _ia, _da, _ib, _db = ref.reference("same", psdr.launch_plan)
    cd = psdr.ChamferDistance(squared=squared)
    for _label, w in CONFIGS:
        cd.weights = w
        loss, terms, gx, gy = _call(cd, x, y)
        assert loss == 0 and not terms.any() and not gx.any() and not gy.any()
        assert np.isfinite(gx).all() and np.isfinite(gy).all()


@pytest.mark.parametrize("squared", [True, False])
@pytest.mark.parametrize("name", ["generic", "hub", "lattice"])
def test_a_direction_of_weight_zero_is_left_out(psdr, name, squared):
    """its value is exactly 0, and the gradients with one direction off are bit-equal to that direction's alone: the two directions' gradients are added once, so the
    float32 sum of the single-direction gradients IS the gradient with both on"""
    x, y, _ia, _da, _ib, _db = ref.reference(name, psdr.launch_plan)
    cd = psdr.ChamferDistance(squared=squared)
    w = (0.75, 1.5)
    cd.weights = (w[0], 0.0)
    a = _call(cd, x, y)
    cd.weights = (0.0, w[1])
    b = _call(cd, x, y)
    assert a[1][1] == 0 and b[1][0] == 0 and a[1][0] > 0 and b[1][1] > 0 and a[0] == np.float32(w[0]) * a[1][0] and b[0] == np.float32(w[1]) * b[1][1]
    assert np.abs(a[2]).max() > 0 and np.abs(a[3]).max() > 0 and np.abs(b[2]).max() > 0 and np.abs(b[3]).max() > 0
    cd.weights = w
    both = _call(cd, x, y)
    assert both[1][0] == a[1][0] and both[1][1] == b[1][1] and np.float32(both[0]) == np.float32(a[0]) + np.float32(b[0])
    assert _bits(both[2]) == _bits(a[2] + b[2]) and _bits(both[3]) == _bits(a[3] + b[3]) and both[2].dtype == np.float32
    cd.weights = (0.0, 0.0)
    loss, terms, gx, gy = _call(cd, x, y)
    assert loss == 0 and not terms.any() and not gx.any() and not gy.any()
    # a direction that is off is not evaluated: the gradient of the other one alone equals the checker's statement of it within the rule (test_accuracy_rule), and a
    # second object with that single weight gives the same bits
    other = psdr.ChamferDistance(weights=(w[0], 0.0), squared=squared)
    again = _call(other, x, y)
    assert again[0] == a[0] and _bits(again[2]) == _bits(a[2]) and _bits(again[3]) == _bits(a[3])


def test_hub_of_300_members(psdr):
    """300 points of y share b(j) = 0, more than a workgroup's 256 lanes: x_0 gathers them in ascending j, and the gradient obeys the rule"""
    x, y, ia, _da, ib, _db = ref.reference("hub", psdr.launch_plan)
    assert (ib == 0).sum() >= 300 > 256
    worst = {}
    for squared in (True, False):
        cd = psdr.ChamferDistance(weights=(0.0, 1.0), squared=squared)
        loss, terms, gx, gy = _call(cd, x, y)
        f64, f32 = ref.evaluate(x, y, ia, ib, (0.0, 1.0), squared), ref.evaluate(x, y, ia, ib, (0.0, 1.0), squared, np.float32)
        _held("hub, squared = %s: dx of the hub" % squared, worst, "hub dx", gx[0], f32["gx"][0], f64["gx"][0])
        _held("hub, squared = %s: dx" % squared, worst, "dx", gx, f32["gx"], f64["gx"])
        _held("hub, squared = %s: dy" % squared, worst, "dy", gy, f32["gy"], f64["gy"])
    print("hub: worst e_gpu / max(e_32, u G): %s" % ", ".join("%s %.2f" % kv for kv in sorted(worst.items())))


def test_ten_calls_return_identical_bits(psdr):
    """the multi-slice case: the loss, both gradients, the indices and the distances"""
    import torch
    x, y, _ia, _da, _ib, _db = ref.reference("generic", psdr.launch_plan)
    assert psdr.launch_plan(len(x), len(y)).slices >= 3 and psdr.launch_plan(len(y), len(x)).slices >= 1
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    cd = psdr.ChamferDistance(weights=(1.0, 0.5), squared=False)
    runs = []
    for _ in range(10):
        loss, gx, gy = cd.value_and_grad(xd, yd)
        runs.append(tuple(_bits(t.cpu().numpy()) for t in (loss, cd.terms, gx, gy) + cd.nearest))
    assert all(r == runs[0] for r in runs[1:])
    xq, yq, _a, _b, _c, _d = ref.reference("one_query", psdr.launch_plan)
    xd, yd = torch.from_numpy(xq).cuda(), torch.from_numpy(yq).cuda()
    first = tuple(_bits(t.cpu().numpy()) for t in psdr.nearest_points(xd, yd))
    assert all(tuple(_bits(t.cpu().numpy()) for t in psdr.nearest_points(xd, yd)) == first for _ in range(9))


# ---- streams

@pytest.mark.parametrize("form", ("S", "default"))
def test_streams(psdr, form):
    """both forms of the delayed producer on cd(x, y) plus its backward: x and y rolled along their first axis are the decoys"""
    import torch
    x, y, _ia, _da, _ib, _db = ref.reference("generic", psdr.launch_plan)
    cd = psdr.ChamferDistance(weights=(1.0, 0.5))
    sx, sy = Slot(torch, x), Slot(torch, y)
    fetch = lambda t: tuple(a.cpu().numpy() for a in t)
    call = lambda: cd.value_and_grad(sx.buf, sy.buf) + (cd.terms,) + cd.nearest
    base = run_plain(torch, [sx, sy], call, fetch)
    import stream_cases as sc_
    for k, (dx_, dy_) in enumerate(((sc_.decoy_of(x), y), (x, sc_.decoy_of(y)))):    # (each decoy is told apart: the rolled set's own gradient is rolled with it)
        decoy = _call(cd, dx_, dy_)
        assert _bits(decoy[2 + k]) != _bits(base[1 + k])
    S = torch.cuda.Stream()

    # autograd under the stream first (backward waits on the host for the engine's thread: no self-check)
    def autograd():
        lx, ly = sx.buf.clone().requires_grad_(), sy.buf.clone().requires_grad_()
        cd(lx, ly).backward()
        return (lx.grad, ly.grad)
    got = run_on_stream(torch, S, form, [sx, sy], autograd, fetch, returns_early=False)
    assert _bits(got[0]) == _bits(base[1]) and _bits(got[1]) == _bits(base[2])
    # the Python layer returns without a synchronisation: the delay is still running when it does
    got = run_on_stream(torch, S, form, [sx, sy], call, fetch)
    assert all(_bits(a) == _bits(b) for a, b in zip(got, base))
    got = run_on_stream(torch, S, form, [sx, sy], lambda: psdr.nearest_points(sx.buf, sy.buf), fetch)
    assert _bits(got[0]) == _bits(base[4]) and _bits(got[1]) == _bits(base[5])


@pytest.mark.parametrize("form", ("S", "default"))
def test_sampler_streams(psdr, form):
    """both forms on sampler(v) and on its transpose"""
    import torch
    v, f = ref.bunny()
    sam = psdr.SurfaceSampler(f, len(v), num_points=3000, seed=1).resample(v)
    g = ref._uniform(3000, 31)
    sv, sg = Slot(torch, v), Slot(torch, g)
    fetch = lambda t: t.cpu().numpy()
    base = run_plain(torch, [sv], lambda: sam(sv.buf), fetch)
    base_t = run_plain(torch, [sg], lambda: sam.transpose(sg.buf), fetch)
    rb, col, w = sam.csr()
    want = (w.reshape(-1, 3, 1).astype(np.float64) * v[col.reshape(-1, 3)]).sum(1)
    assert np.abs(base - want).max() <= 4 * ref.U * np.abs(v).max()
    S = torch.cuda.Stream()

    # autograd under the stream first (backward waits on the host for the engine's thread, and the first launch on a new stream takes milliseconds: no self-check)
    def autograd():
        leaf = sv.buf.clone().requires_grad_()
        (sam(leaf) * sg._true).sum().backward()
        return leaf.grad
    assert _bits(run_on_stream(torch, S, form, [sv], autograd, fetch, returns_early=False)) == _bits(base_t)
    assert _bits(run_on_stream(torch, S, form, [sv], lambda: sam(sv.buf), fetch)) == _bits(base)
    assert _bits(run_on_stream(torch, S, form, [sg], lambda: sam.transpose(sg.buf), fetch)) == _bits(base_t)


# ---- autograd

def test_autograd_scales_the_forward_gradients(psdr):
    import torch
    x, y, _ia, _da, _ib, _db = ref.reference("generic", psdr.launch_plan)
    cd = psdr.ChamferDistance(weights=(1.0, 0.5))
    loss, gx, gy = cd.value_and_grad(torch.from_numpy(x), torch.from_numpy(y))
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda and not loss.requires_grad and not gx.requires_grad and cd.terms.shape == (2,)
    lx, ly = torch.from_numpy(x).cuda().requires_grad_(), torch.from_numpy(y).cuda().requires_grad_()
    out = cd(lx, ly)
    assert out.dim() == 0 and out.dtype == torch.float32 and out.is_cuda and out.item() == loss.item() and not cd.terms.requires_grad
    (3 * out).backward()
    assert torch.equal(lx.grad, 3 * gx) and torch.equal(ly.grad, 3 * gy)
    # x on the host in float64, y a constant: the gradient returns to x's device and dtype
    hx = torch.from_numpy(x.astype(np.float64)).requires_grad_()
    (3 * cd(hx, torch.from_numpy(y))).backward()
    assert hx.grad.dtype == torch.float64 and not hx.grad.is_cuda and torch.equal(hx.grad, (3 * gx).cpu().double())
    # the plain attributes are read at every call
    cd.weights, cd.squared = (0.0, 1.0), False
    assert cd(lx, ly).item() == cd.terms[1].item() and cd.terms[0].item() == 0
    cd.weights = (1.0, -1.0)
    with pytest.raises(ValueError):
        cd(lx, ly)


def test_autograd_through_the_sampler(psdr):
    """cd(sam(v), target).backward() reaches v and equals the sampler's transpose applied to the dx of value_and_grad, bit for bit"""
    import torch
    v, f = ref.bunny()
    sam = psdr.SurfaceSampler(f, len(v), num_points=2000, seed=2).resample(v)
    target = torch.from_numpy(ref._uniform(1500, 32, 0.0, 1.0)).cuda()
    cd = psdr.ChamferDistance()
    leaf = torch.from_numpy(v).cuda().requires_grad_()
    pts = sam(leaf)
    assert pts.shape == (2000, 3) and pts.requires_grad
    cd(pts, target).backward()
    _loss, dx, _dy = cd.value_and_grad(sam(leaf.detach()), target)
    want = sam.transpose(dx)
    assert dx.abs().max() > 0 and torch.equal(leaf.grad, want)
    # the transpose on the device is the host CSR's transpose: against float64 within the rounding of a row's sum
    trb, tcol, tw = sam.csr(transpose=True)
    rows = np.repeat(np.arange(len(v)), np.diff(trb))
    ref64 = np.zeros((len(v), 3))
    np.add.at(ref64, rows, tw[:, None].astype(np.float64) * dx.cpu().numpy().astype(np.float64)[tcol])
    mag = np.zeros((len(v), 3))
    np.add.at(mag, rows, np.abs(tw[:, None].astype(np.float64) * dx.cpu().numpy().astype(np.float64)[tcol]))
    assert (np.abs(want.cpu().numpy() - ref64) <= (np.diff(trb).max() + 2) * ref.U * mag.max()).all()


def test_autograd_through_subdivision_and_the_preconditioner(psdr):
    """cd(sam(sub.refine(pre.from_differential(u))), target): the gradient reaches u, and equals the chain applied by hand within the solve's tolerance"""
    import torch
    import meshreg_ref
    faces, n, c0 = meshreg_ref.case("grid9")
    pre = psdr.LaplacianPreconditioner(np.array(faces), n)
    sub = psdr.Subdivision(np.array(faces), n, levels=1)
    fine = sub.refine(torch.from_numpy(c0)).cpu().numpy()
    sam = psdr.SurfaceSampler(sub.faces, sub.num_vertices_out, num_points=1500, seed=3).resample(fine)
    target = torch.from_numpy(fine + np.float32(0.3)).cuda()
    cd = psdr.ChamferDistance()
    u = pre.to_differential(torch.from_numpy(c0)).detach().requires_grad_()
    cd(sam(sub.refine(pre.from_differential(u))), target).backward()
    _loss, dx, _dy = cd.value_and_grad(sam(sub.refine(pre.from_differential(u.detach()))), target)
    g = sub.restrict(sam.transpose(dx))
    want = pre.from_differential(g)
    assert g.norm() > 0 and (u.grad - want).norm().item() <= 2 * pre.rtol * g.norm().item()


def test_shape_recovery(psdr):
    """the bunny's vertices displaced by a smooth offset of 5 % of the bounding box, 50 steps of AdamUniform on cd(sam(v), sam_target(V_bunny)) with a resample every 10
    steps: the Chamfer distance falls below half of the starting distance, both measured here with the same sampler state rule (a fresh resample of the moving mesh)"""
    import torch
    V, f = ref.bunny()
    box = float((V.max(0) - V.min(0)).max())
    offset = 0.05 * box * np.stack([np.sin(3.0 * V[:, 1] + 1.0), np.sin(3.0 * V[:, 2] + 2.0), np.cos(3.0 * V[:, 0])], 1)
    assert 0.03 * box <= np.linalg.norm(offset, axis=1).max() <= 0.05 * box * np.sqrt(3.0)
    target = psdr.SurfaceSampler(f, len(V), num_points=10000, seed=5).resample(V)(torch.from_numpy(V)).detach()
    v = torch.from_numpy((V + offset).astype(np.float32)).cuda().requires_grad_()
    sam = psdr.SurfaceSampler(f, len(V), num_points=10000, seed=6)
    cd = psdr.ChamferDistance()
    opt = psdr.AdamUniform([v], lr=0.002)
    start = None
    for step in range(50):
        if step % 10 == 0:
            sam.resample(v.detach())
        opt.zero_grad()
        loss = cd(sam(v), target)
        loss.backward()
        opt.step()
        if start is None:
            start = loss.item()
    sam.resample(v.detach())
    end = cd(sam(v.detach()), target).item()
    print("shape recovery: Chamfer distance %.4g -> %.4g (ratio %.3f)" % (start, end, end / start))
    assert np.isfinite(end) and end < 0.5 * start, "the Chamfer distance fell from %.4g to %.4g only" % (start, end)
