"""GPU tests of the signed distance (psdr_jit_amd/sdf.py, csrc/hip/sdf.hip) against the numpy checker tests/sdf_ref.py.

Per case and per array by the rule of tests/test_gpu_meshreg.py and tests/test_gpu_pointmesh.py, e_gpu <= 4 max(e_32, u G), u = 2^-24, against float64:
    w                    the winding number; G = max_i sum_f |theta(p_i, f)| / (2 pi), e_32 the deviation of the float32 checker (one ascending sum)
    s                    the signed distance against float64's, G = max |s|, e_32 the float32 checker's (its own nearest face, its own sign)
    d / dpoints, d / dv  the vector-Jacobian product for a random g against the float64 evaluation THROUGH THE DEVICE'S INDICES AND SIGN
dist2, face and bary are not measured again: they equal closest_points_on_mesh's bit for bit, which tests/test_gpu_pointmesh.py holds to the rule.  The sign: inside equals
float64's at every point whose |w64 - 1 / 2| exceeds the rule's yardstick for the case; the points inside that band are left out and may be at most 1 % of a case.  Every test
prints the worst ratio it saw per array.

Measured on an MI355X, the worst e_gpu / max(e_32, u G) over all cases: w 2.49 (F = 1: the library atan2f against a correctly rounded one, nothing
else contributes), at most 1.00 elsewhere (cubes); s 1.00, d / dpoints 1.00, d / dv 1.00 (the float32 checker's own error: the device has its operations).  No point of any
closed case lay in the band.  The penetration penalty fell from 2.088 to 1.0e-6, the vertices inside from 967 to 4.

Then the exact cases (points on vertices, the tie rule), repeatability, both stream forms of tests/stream_cases.py, autograd, and a penetration penalty between two bunnies."""
import numpy as np
import pytest

import pointmesh_ref as pref
import sdf_ref as ref
from stream_cases import Slot, run_on_stream, run_plain

pytestmark = pytest.mark.gpu

NS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)
NAMED = ("bunny", "near", "regions", "cubes", "degenerate")


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


def _held(what, worst, key, dev, f32, f64, G=None):
    r, e_gpu, e_32, G = ref.ratio(dev, f32, f64, G)
    worst[key] = max(worst.get(key, 0.0), r)
    assert np.isfinite(np.asarray(dev)).all(), what
    assert r <= 4.0, "%s, %s: e_gpu = %.3g, e_32 = %.3g, u G = %.3g: ratio %.3g > 4" % (what, key, e_gpu, e_32, ref.U * G, r)


def _report(what, worst):
    print("%s: worst e_gpu / max(e_32, u G): %s" % (what, ", ".join("%s %.2f" % kv for kv in sorted(worst.items()))))


def _band(r):
    """the points of a reference whose float64 |w| lies within the rule's yardstick of 1 / 2: their sign is not asserted"""
    yard = max(np.abs(r["w32"] - r["w64"]).max(), ref.U * r["G"].max())
    return np.abs(np.abs(r["w64"]) - 0.5) <= yard


# ---- the plan's boundaries

@pytest.mark.parametrize("which", range(5))
def test_sizes_on_the_edges_of_the_plan(psdr, which):
    """every N on the wave's, the workgroup's and the queries-per-lane edges against F in {1, tile - 1, tile, tile + 1, 2 tile + 1}, tile read from the plan, on leading blocks
    of pointmesh_ref's sweep: w under the rule; dist2, face and bary are closest_points_on_mesh's bits; s s equals dist2 within one rounding of the square root.  The lattice
    is open: no sign is asserted"""
    plan = psdr.launch_plan_pm
    tile = plan(1, 1).tile
    fs = (1, tile - 1, tile, tile + 1, 2 * tile + 1)
    F = fs[which]
    assert len({plan(n, 1).queries_per_lane for n in NS}) >= 2 and plan(1, fs[-1]).slices >= 3
    p_all, v, f_all, W64, G, W32 = ref.sweep_reference(max(NS), fs[-1])
    f = f_all[:F]
    worst = {}
    for N in NS:
        p = p_all[:N]
        res = psdr.signed_distance(_t(p), _t(v), f)
        what = "N = %d, F = %d, plan %s" % (N, F, tuple(plan(N, F)))
        assert res.winding.shape == (N,) and res.sdf.shape == (N,)
        _held(what, worst, "w", _np(res.winding), W32[:N, F - 1], W64[:N, F - 1], G[:N, F - 1])
        assert _bits(_np(psdr.winding_number(_t(p), _t(v), f))) == _bits(_np(res.winding)), what
        near = psdr.closest_points_on_mesh(_t(p), _t(v), f)
        assert all(_bits(_np(a)) == _bits(_np(b)) for a, b in zip((res.face, res.bary, res.dist2), near)), what
        s, d2 = _np(res.sdf).astype(np.float64), _np(res.dist2).astype(np.float64)
        assert np.isfinite(s).all() and (np.abs(s * s - d2) <= (2.0 * ref.U + ref.U ** 2) * d2).all(), what          # s = sqrt(d2) (1 + e), |e| <= u: s s = d2 (1 + e)^2
        assert _bits(np.abs(_np(res.sdf))) == _bits(np.sqrt(_np(res.dist2))), what
        assert ((_np(res.sdf) < 0) == (_np(res.winding) > 0.5))[_np(res.dist2) > 0].all(), what
    _report("F = %d" % F, worst)


# ---- the named cases

def _evaluate(psdr, r, orientation=1, seed=71):
    """one sd.vjp on a reference -> (w, s, inside, gp, gv, face, g) as numpy"""
    sd = psdr.SignedDistance(r["f"], len(r["v"]), orientation=orientation)
    g = np.random.default_rng(seed).uniform(-1.0, 1.0, len(r["p"])).astype(np.float32)
    s, gp, gv = sd.vjp(_t(r["p"]), _t(r["v"]), _t(g))
    w = _np(sd.winding)
    return w, _np(s), np.float32(orientation) * w > 0.5, _np(gp), _np(gv), _np(sd.nearest.face), g


@pytest.mark.parametrize("name", NAMED)
def test_accuracy_rule(psdr, name):
    """w, s and the vector-Jacobian product under the rule, everything finite, and the sign against float64's outside the yardstick band"""
    r = ref.reference(name)
    p, v, f = r["p"], r["v"], r["f"]
    w, s, inside, gp, gv, face, g = _evaluate(psdr, r)
    worst = {}
    _held(name, worst, "w", w, r["w32"], r["w64"], r["G"])
    band = _band(r)
    in64, in32 = ref.inside_of(r["w64"]), ref.inside_of(r["w32"])
    print("%s: %d of %d points within the yardstick of 1 / 2, %d inside" % (name, band.sum(), len(band), in64.sum()))
    assert band.mean() <= 0.01, "a condition on the case: %d of %d points lie in the band" % (band.sum(), len(band))
    assert np.array_equal(inside[~band], in64[~band]), "%s: the sign differs from float64's at %s" % (name, np.nonzero((inside != in64) & ~band)[0][:8])
    assert in64.any() and not in64.all()
    # s: in the band the magnitudes are compared
    s64, s32 = ref.signed(r["c64"].dist2_p, in64), ref.signed(r["c32"].dist2_p, in32)
    fold = lambda a: np.where(band, np.abs(a), a)
    _held(name, worst, "s", fold(s), fold(s32), fold(s64))
    _s64, gp64, gv64 = ref.vjp(p, v, f, face, inside, g, np.float64)
    _s32, gp32, gv32 = ref.vjp(p, v, f, face, inside, g, np.float32)
    _held(name, worst, "d/dpoints", gp, gp32, gp64)
    _held(name, worst, "d/dv", gv, gv32, gv64)
    assert all(np.isfinite(a).all() for a in (w, s, gp, gv)) and np.abs(gp).max() > 0 and np.abs(gv).max() > 0
    if name == "cubes":
        assert (np.abs(r["w64"] - 2) < 1e-9).sum() >= 10 and (np.round(w[~band]) == np.round(r["w64"][~band])).all()          # (the overlap is reached: w = 2 there)
    _report(name, worst)


@pytest.mark.parametrize("name", ("octahedron", "cubes", "bunny", "degenerate"))
def test_reversed_winding(psdr, name):
    """every face reversed: with orientation = -1 the same inside as the mesh as it is with +1, and the same s - under the rule, not bit for bit: the reversed face hands
    the point-to-mesh cascade its corners in another order, which sums its interior denominator in another association; with orientation = +1 every point reports outside"""
    r, rr = ref.reference(name), ref.reference(name, flipped=True)
    w, s, inside, _gp, _gv, _face, _g = _evaluate(psdr, r)
    wr, sr, inside_r, _gp, _gv, _face, _g = _evaluate(psdr, rr, orientation=-1)
    worst = {}
    _held(name + " reversed", worst, "w", wr, rr["w32"], rr["w64"], rr["G"])
    keep = ~(_band(r) | _band(rr))
    assert keep.mean() >= 0.99 and inside.any()
    assert np.array_equal(inside_r[keep], inside[keep])
    in64 = ref.inside_of(r["w64"])
    assert np.array_equal(ref.inside_of(rr["w64"], -1)[keep], in64[keep])
    fold = lambda a: np.where(keep, a, np.abs(a))
    s64 = ref.signed(rr["c64"].dist2_p, in64)
    _held(name + " reversed", worst, "s", fold(sr), fold(ref.signed(rr["c32"].dist2_p, ref.inside_of(rr["w32"], -1))), fold(s64))
    _held(name, worst, "s", fold(s), fold(ref.signed(r["c32"].dist2_p, ref.inside_of(r["w32"]))), fold(s64))          # (one float64 s serves both windings)
    res = psdr.signed_distance(_t(rr["p"]), _t(rr["v"]), rr["f"], orientation=1)
    assert (_np(res.sdf) >= 0).all() and not (_np(res.winding) > 0.5).any()
    assert _bits(_np(res.winding)) == _bits(wr)
    _report(name + " reversed", worst)


# ---- exact cases

def test_points_on_the_vertices(psdr):
    """the points are the mesh's own vertices: s == 0 and both gradients are exactly 0 (s may be -0 where the vertex counts as inside)"""
    v, f = pref.bunny()
    sd = psdr.SignedDistance(f, len(v))
    p = v[np.unique(f)]
    s, gp, gv = (_np(a) for a in sd.vjp(_t(p), _t(v), _t(np.ones(len(p), np.float32))))
    assert not s.any() and not gp.any() and not gv.any() and np.isfinite(_np(sd.winding)).all()
    assert not _np(sd.nearest.dist2).any()


def test_the_lower_face_wins_a_tie(psdr):
    """a direction-0 tie keeps the point-to-mesh rule: an exact copy of the winning face at a higher index, in the same tile and in another slice - the lower index is
    reported, and the arrays are closest_points_on_mesh's"""
    plan = psdr.launch_plan_pm
    tile = plan(1, 1).tile
    N, F = 300, 4 * tile + 9
    assert plan(N, F).slices >= 3
    v0, f0 = pref.lattice(F)
    v0 = v0 + np.float32([5.0, 0.0, 0.0])
    tri = np.float32([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.0, 0.5, 0.1]])
    v = np.concatenate([v0, tri])
    ids = len(v0) + np.arange(3)
    p = (np.float32([0.15, 0.15, 0.1]) + np.float32(0.05) * np.random.default_rng(51).uniform(-1, 1, (N, 3))).astype(np.float32)
    for at, copy_at in ((5, 7), (5, 5 + plan(N, F).slice_len), (0, F - 1)):
        f = f0.copy()
        f[at] = f[copy_at] = ids
        res = psdr.signed_distance(_t(p), _t(v), f)
        assert (_np(res.face) == at).all(), (at, copy_at, np.unique(_np(res.face)))
        near = psdr.closest_points_on_mesh(_t(p), _t(v), f)
        assert all(_bits(_np(a)) == _bits(_np(b)) for a, b in zip((res.face, res.bary, res.dist2), near))


# ---- repeatability, streams

def test_ten_calls_return_identical_bits(psdr):
    import torch
    r = ref.reference("regions")
    assert psdr.launch_plan_pm(len(r["p"]), len(r["f"])).slices >= 3
    pd, vd = _t(r["p"]).cuda(), _t(r["v"]).cuda()
    g = _t(np.random.default_rng(72).uniform(-1, 1, len(r["p"])).astype(np.float32)).cuda()
    sd = psdr.SignedDistance(r["f"], len(r["v"]))
    runs = []
    for _ in range(10):
        s, gp, gv = sd.vjp(pd, vd, g)
        runs.append(tuple(_bits(_np(t)) for t in (sd.winding, s, gp, gv)))
    assert all(x == runs[0] for x in runs[1:])
    fd = _t(r["f"].astype(np.int32)).cuda()
    assert all(_bits(_np(psdr.winding_number(pd, vd, fd))) == runs[0][0] for _ in range(3))
    assert torch.cuda.is_available()


@pytest.mark.parametrize("form", ("S", "default"))
def test_streams(psdr, form):
    """both forms of the delayed producer on sd(points, v), its backward and winding_number: points and v rolled along their first axis are the decoys"""
    import torch
    import stream_cases as sc_
    r = ref.reference("near")
    p, v, f = r["p"], r["v"], r["f"]
    sd = psdr.SignedDistance(f, len(v))
    sp, sv = Slot(torch, p), Slot(torch, v)
    g = _t(np.random.default_rng(73).uniform(-1, 1, len(p)).astype(np.float32)).cuda()
    fd = _t(f.astype(np.int32)).cuda()
    fetch = lambda t: tuple(_np(a) for a in t)

    def call():
        s = sd(sp.buf, sv.buf)
        return (s, sd.winding)
    base = run_plain(torch, [sp, sv], lambda: sd.vjp(sp.buf, sv.buf, g) + (sd.winding,), fetch)
    for dp_, dv_ in ((sc_.decoy_of(p), v), (p, sc_.decoy_of(v))):          # (each decoy is told apart)
        assert _bits(_np(sd.vjp(_t(dp_), _t(dv_), g)[0])) != _bits(base[0])
    S = torch.cuda.Stream()

    # autograd under the stream first (backward waits on the host for the engine's thread: no self-check)
    def autograd():
        lp, lv = sp.buf.clone().requires_grad_(), sv.buf.clone().requires_grad_()
        sd(lp, lv).backward(g)
        return (lp.grad, lv.grad)
    got = run_on_stream(torch, S, form, [sp, sv], autograd, fetch, returns_early=False)
    assert _bits(got[0]) == _bits(base[1]) and _bits(got[1]) == _bits(base[2])
    # the Python layer returns without a synchronisation: the delay is still running when it does
    got = run_on_stream(torch, S, form, [sp, sv], call, fetch)
    assert _bits(got[0]) == _bits(base[0]) and _bits(got[1]) == _bits(base[3])
    got = run_on_stream(torch, S, form, [sp, sv], lambda: (psdr.winding_number(sp.buf, sv.buf, fd),), fetch)
    assert _bits(got[0]) == _bits(base[3])


# ---- autograd

def test_autograd_equals_vjp(psdr):
    import torch
    r = ref.reference("near")
    p, v, f = r["p"], r["v"], r["f"]
    sd = psdr.SignedDistance(f, len(v))
    g = _t(np.random.default_rng(74).uniform(-1, 1, len(p)).astype(np.float32)).cuda()
    s, gp, gv = sd.vjp(_t(p), _t(v), g)
    assert s.shape == (len(p),) and s.dtype == torch.float32 and s.is_cuda and not s.requires_grad and not gp.requires_grad and gp.shape == (len(p), 3) and gv.shape == (len(v), 3)
    lp, lv = _t(p).cuda().requires_grad_(), _t(v).cuda().requires_grad_()
    out = sd(lp, lv)
    assert out.shape == (len(p),) and out.dtype == torch.float32 and out.is_cuda and torch.equal(out.detach(), s)
    assert not sd.winding.requires_grad and not sd.nearest.bary.requires_grad and sd.winding.shape == (len(p),)
    out.backward(g)
    assert torch.equal(lp.grad, gp) and torch.equal(lv.grad, gv)
    # v on the host in float64, the points a constant: the gradient returns to v's device and dtype
    hv = _t(v.astype(np.float64)).requires_grad_()
    sd(_t(p), hv).backward(g)
    assert hv.grad.dtype == torch.float64 and not hv.grad.is_cuda and torch.equal(hv.grad, gv.cpu().double())
    # the function form gives the same arrays
    res = psdr.signed_distance(_t(p), _t(v), f)
    assert torch.equal(res.sdf, s) and torch.equal(res.winding, sd.winding) and all(torch.equal(a, b) for a, b in zip(res[2:], sd.nearest))
    # orientation is read at every call
    sd.orientation = -1
    assert (sd(lp, lv) >= 0).all()
    sd.orientation = 3
    with pytest.raises(ValueError):
        sd(lp, lv)


def test_autograd_through_subdivision_and_the_preconditioner(psdr):
    """sd(points, sub.refine(c)).backward(g) and sd(points, pre.from_differential(u)).backward(g) reach c and u; the vertex gradient that enters them is vjp's, bit for bit"""
    import torch
    import meshreg_ref
    faces, n, c0 = meshreg_ref.case("grid9")
    sub = psdr.Subdivision(np.array(faces), n, levels=1)
    fine = _np(sub.refine(_t(c0)))
    points = _t((fine[::2] + np.float32([0.02, -0.03, 0.15])).astype(np.float32)).cuda()
    g = _t(np.random.default_rng(75).uniform(0.5, 1.0, len(points)).astype(np.float32)).cuda()
    sd = psdr.SignedDistance(sub.faces, sub.num_vertices_out)
    c = _t(c0).cuda().requires_grad_()
    sd(points, sub.refine(c)).backward(g)
    _s, _gp, gv = sd.vjp(points, sub.refine(c.detach()), g)
    assert gv.abs().max() > 0 and torch.equal(c.grad, sub.restrict(gv))
    pre = psdr.LaplacianPreconditioner(np.array(faces), n)
    coarse = psdr.SignedDistance(np.array(faces), n)
    pts = _t((c0 + np.float32([0.02, -0.03, 0.15])).astype(np.float32)).cuda()
    gc = _t(np.random.default_rng(76).uniform(0.5, 1.0, len(pts)).astype(np.float32)).cuda()
    u = pre.to_differential(_t(c0)).detach().requires_grad_()
    coarse(pts, pre.from_differential(u)).backward(gc)
    _s, _gp, gu = coarse.vjp(pts, pre.from_differential(u.detach()), gc)
    want = pre.from_differential(gu)
    assert gu.norm() > 0 and (u.grad - want).norm().item() <= 2 * pre.rtol * gu.norm().item()


# ---- use

def test_penetration_penalty_pushes_a_copy_out(psdr):
    """the bunny and a copy translated by 10 % of its box: 30 steps of AdamUniform on sum relu(-sd(v_copy, v_bunny))^2 with only the copy moving.  The penalty ends below half
    of its start and the count of inside vertices falls.  lr: AdamUniform moves a vertex by lr times its gradient over the largest, a gradient is twice the depth, and the
    deepest vertex lies 10 % of the box inside, so a depth decays by about exp(-30 lr / 0.1) - lr = 0.005 leaves a fifth of every depth, far below the bar"""
    import torch
    V, f = pref.bunny()
    box = float((V.max(0) - V.min(0)).max())
    vb = _t(V).cuda()
    vc = _t((V + np.float32([0.1 * box, 0.0, 0.0])).astype(np.float32)).cuda().requires_grad_()
    sd = psdr.SignedDistance(f, len(V))
    opt = psdr.AdamUniform([vc], lr=0.005)
    penalty = lambda: torch.relu(-sd(vc, vb)).square().sum()
    start, inside_start = penalty().item(), int((sd.winding > 0.5).sum().item())
    for _step in range(30):
        opt.zero_grad()
        penalty().backward()
        opt.step()
    end, inside_end = penalty().item(), int((sd.winding > 0.5).sum().item())
    print("penetration penalty %.4g -> %.4g (ratio %.3f), vertices inside %d -> %d" % (start, end, end / start, inside_start, inside_end))
    assert np.isfinite(end) and start > 0 and end < 0.5 * start and inside_end < inside_start
