"""GPU tests of the lattice regularisers (psdr_jit_amd/latreg.py, csrc/hip/latreg.hip) against the numpy statement of the definition in
tests/latreg_ref.py.

The accuracy rule is that of tests/test_gpu_meshreg.py: e_gpu <= 4 max(e_32, u G), u = 2^-24, G the largest magnitude of the float64 result, e_32 the error of the float32
checker against float64 - per case, per term alone and with all terms on, for the value and for the gradient.  The shapes: the smallest lattice, strides that all differ,
shapes read from launch_plan_lr one below, on and one above every extent of a workgroup's tile and its double, and 33^3; anisotropic spacing; a sphere's distance plus noise
and pure noise; sign_scale 1 and 40.  Then the exact cases bit for bit, the crossing count against marching tetrahedra's, the behaviour of the Python surface, both stream
forms of tests/stream_cases.py, and one DMTet step.

Measured on an MI355X, the worst e_gpu / max(e_32, u G) over all accuracy cases: eikonal 1.84, laplacian 2.25, sign 1.30, the loss with all terms on
2.90, the gradient 1.00 / 1.00 / 1.37 for a term alone and 1.45 with all on; +-c 1.86 (k = 1) and 2.06 (k = 40).  The gradient's 1.00 is the float32 checker's own error (the
device has the checker's operations in the checker's order); the values differ from the checker in the order of their sums."""
import numpy as np
import pytest

import latreg_ref as ref
from stream_cases import Slot, run_on_stream, run_plain

pytestmark = pytest.mark.gpu

ALL = (0.7, 0.02, 0.3)          # every term on, weights that differ
SINGLE = {"eikonal": (1.0, 0.0, 0.0), "laplacian": (0.0, 1.0, 0.0), "sign": (0.0, 0.0, 1.0)}
N_SHAPES = 12                   # len(ref.accuracy_shapes(tile)), asserted below


@pytest.fixture(scope="module")
def psdr():
    import __graft_entry__
    __graft_entry__.build()
    import psdr_jit_amd
    return psdr_jit_amd


@pytest.fixture(scope="module")
def cases(psdr):
    tile = psdr.launch_plan_lr((2, 2, 2)).tile
    shapes = ref.accuracy_shapes(tile)
    assert len(shapes) == N_SHAPES and shapes[5] == tuple(t - 1 for t in tile) and shapes[10] == tuple(2 * t + 1 for t in tile)
    return ref.accuracy_cases(tile)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a))


def _np(t):
    return t.detach().cpu().numpy()


def _held(what, worst, key, dev, f32, f64):
    r, e_gpu, e_32, G = ref.ratio(dev, f32, f64)
    worst[key] = max(worst.get(key, 0.0), r)
    assert np.isfinite(np.asarray(dev)).all(), what
    assert r <= 4.0, "%s, %s: e_gpu = %.3g, e_32 = %.3g, u G = %.3g: ratio %.3g > 4" % (what, key, e_gpu, e_32, ref.U * G, r)


def _report(what, worst):
    print("%s: worst e_gpu / max(e_32, u G): %s" % (what, ", ".join("%s %.2f" % kv for kv in sorted(worst.items()))))


def _eval(psdr, shape, spacing, weights, k, sdf):
    lr = psdr.LatticeRegularizer(shape, spacing, weights=weights, sign_scale=k)
    loss, grad = lr.value_and_grad(_t(sdf))
    return float(_np(loss)), _np(lr.terms), _np(grad), int(_np(lr.num_crossings)[0]), lr


# ---- 1. the accuracy rule

@pytest.mark.parametrize("index", range(N_SHAPES))
def test_accuracy_rule(psdr, cases, index):
    worst = {}
    for name, shape, sdf in cases[2 * index:2 * index + 2]:
        plan = psdr.launch_plan_lr(shape)
        assert plan.num_lattice == len(sdf)
        configs = [("eikonal", SINGLE["eikonal"], 1.0), ("laplacian", SINGLE["laplacian"], 1.0)]
        configs += [("sign k=%g" % k, SINGLE["sign"], k) for k in ref.SIGN_SCALES] + [("all k=%g" % k, ALL, k) for k in ref.SIGN_SCALES]
        for label, weights, k in configs:
            what = "%s, %s" % (name, label)
            loss, terms, grad, V, _lr = _eval(psdr, shape, ref.ACCURACY_SPACING, weights, k, sdf)
            r32 = ref.reference(sdf, shape, ref.ACCURACY_SPACING, weights, k, np.float32)
            r64 = ref.reference(sdf, shape, ref.ACCURACY_SPACING, weights, k)
            key = label.split(" ")[0]
            assert V == r64["V"], what
            for j, term in enumerate(("eikonal", "laplacian", "sign")):
                if weights[j] > 0:
                    _held(what, worst, "%s.%s" % (key, term), terms[j], r32["terms"][j], r64["terms"][j])
                else:
                    assert terms[j] == 0, what
            _held(what, worst, key + ".loss", loss, r32["loss"], r64["loss"])
            _held(what, worst, key + ".grad", grad, r32["grad"], r64["grad"])
    _report("accuracy %s" % (cases[2 * index][1],), worst)


# ---- 2. the exact cases

EXACT_SHAPE = (35, 9, 6)         # more than one tile along every axis


def test_a_linear_field_is_exactly_zero(psdr):
    P = ref.positions(EXACT_SHAPE, ref.EXACT_SPACING)
    sdf = P[:, 0].astype(np.float32)
    assert np.array_equal(sdf.astype(np.float64), P[:, 0])
    for term in ("eikonal", "laplacian"):
        loss, terms, grad, _V, _lr = _eval(psdr, EXACT_SHAPE, ref.EXACT_SPACING, SINGLE[term], 1.0, sdf)
        assert loss == 0 and not terms.any() and not grad.any(), term
    loss, terms, grad, _V, _lr = _eval(psdr, EXACT_SHAPE, ref.EXACT_SPACING, (1.0, 1.0, 0.0), 1.0, sdf)
    assert loss == 0 and not terms.any() and not grad.any()


def test_a_parabola_has_residual_two(psdr):
    P, X = ref.positions(EXACT_SHAPE, ref.EXACT_SPACING), ref.coords(EXACT_SHAPE)
    sdf = (P[:, 0] ** 2).astype(np.float32)
    assert np.array_equal(sdf.astype(np.float64), P[:, 0] ** 2)
    nv = len(sdf)
    interior = int(((X[:, 0] >= 1) & (X[:, 0] <= EXACT_SHAPE[0] - 2)).sum())
    _loss, terms, grad, _V, _lr = _eval(psdr, EXACT_SHAPE, ref.EXACT_SPACING, SINGLE["laplacian"], 1.0, sdf)
    exact = 4.0 * interior / nv
    print("laplacian of the parabola: %r, 4 (share of Nv) = %r" % (float(terms[1]), exact))
    assert abs(float(terms[1]) - exact) <= np.spacing(np.float32(exact)) / 2 and terms[1] == np.float32(exact)          # one rounding
    # r == 2 on the x-interior vertices: along every axis the gradient (2 / Nv) (-2 r + r + r) / h^2 is exactly 0 where the vertex and both neighbours are interior
    G = grad.reshape(EXACT_SHAPE[2], EXACT_SHAPE[1], EXACT_SHAPE[0])
    assert G[2:-2, 2:-2, 2:-2].size > 0 and not G[2:-2, 2:-2, 2:-2].any() and G[:, :, 0].all()
    assert _bits(grad) == _bits(ref.reference(sdf, EXACT_SHAPE, ref.EXACT_SPACING, SINGLE["laplacian"], 1.0, np.float32)["grad"])


def test_a_constant_field(psdr):
    sdf = np.full(ref.counts(EXACT_SHAPE)[0], 0.75, np.float32)
    loss, terms, grad, V, _lr = _eval(psdr, EXACT_SHAPE, ref.EXACT_SPACING, (1.0, 1.0, 1.0), 1.0, sdf)
    assert terms.tolist() == [1.0, 0.0, 0.0] and loss == 1.0 and V == 0 and not grad.any() and np.isfinite(grad).all()


@pytest.mark.parametrize("k", ref.SIGN_SCALES)
def test_plus_minus_c_with_random_signs(psdr, k):
    worst = {}
    c = np.float32(0.3)
    sdf = np.random.default_rng(4).choice(np.array([-c, c], np.float32), ref.counts(EXACT_SHAPE)[0])
    _loss, terms, _grad, V, _lr = _eval(psdr, EXACT_SHAPE, ref.EXACT_SPACING, SINGLE["sign"], k, sdf)
    kc = float(k) * float(c)
    exact = 2.0 * (kc + np.log1p(np.exp(-kc)))
    f32 = ref.sign_vertices(sdf, EXACT_SHAPE, k, np.float32)[0]
    assert V == ref.sign_edges(sdf, EXACT_SHAPE, k)[1] > 0
    _held("+-c, k = %g" % k, worst, "sign", terms[2], f32, exact)
    _report("+-c, k = %g" % k, worst)


def test_no_crossing(psdr):
    sdf = np.abs(ref.pure_noise(EXACT_SHAPE, 6)) + np.float32(0.1)
    for s in (sdf, -sdf):
        loss, terms, grad, V, _lr = _eval(psdr, EXACT_SHAPE, ref.EXACT_SPACING, SINGLE["sign"], 40.0, s)
        assert loss == 0 and terms[2] == 0 and V == 0 and not grad.any()


# ---- 3. the crossings are marching tetrahedra's vertices

def test_crossings_equal_the_extracted_vertices(psdr):
    shape = (33, 33, 33)
    signs = np.random.default_rng(30).choice(np.array([-1.0, 1.0], np.float32), ref.counts(shape)[0])
    *_rest, V, _lr = _eval(psdr, shape, 0.1, SINGLE["sign"], 1.0, signs)
    topo = psdr.MarchingTetrahedra(shape).extract(_t(signs))
    assert V == topo.num_vertices == int(ref.crossing_counts(signs, shape).sum()) // 2 and V > 0.4 * 7 * len(signs)
    shape = (5, 3, 3)
    plane = (ref.coords(shape)[:, 0] - 2).astype(np.float32)            # exact zeros on the plane x = 2: outside
    *_rest, V, _lr = _eval(psdr, shape, 0.1, SINGLE["sign"], 1.0, plane)
    assert V == psdr.MarchingTetrahedra(shape).extract(_t(plane)).num_vertices > 0


# ---- 4. behaviour

def _case(shape=(37, 10, 7), seed=50):
    return shape, ref.sphere_noise(shape, ref.ACCURACY_SPACING, seed)


def test_a_term_of_weight_zero_reports_zero_and_leaves_the_others(psdr):
    shape, sdf = _case()
    _l, full, _g, V, _lr = _eval(psdr, shape, ref.ACCURACY_SPACING, ALL, 3.0, sdf)
    assert full.all() and V > 0
    for j in range(3):
        w = tuple(0.0 if i == j else x for i, x in enumerate(ALL))
        _l, terms, grad, Vj, _lr = _eval(psdr, shape, ref.ACCURACY_SPACING, w, 3.0, sdf)
        assert terms[j] == 0 and all(_bits(terms[i]) == _bits(full[i]) for i in range(3) if i != j), j
        assert Vj == (0 if j == 2 else V) and np.isfinite(grad).all()
    _l, terms, grad, V0, _lr = _eval(psdr, shape, ref.ACCURACY_SPACING, (0.0, 0.0, 0.0), 3.0, sdf)
    assert _l == 0 and not terms.any() and not grad.any() and V0 == 0


def test_value_only_call_and_five_identical_calls(psdr):
    import torch
    shape, sdf = _case(seed=51)
    lr = psdr.LatticeRegularizer(shape, ref.ACCURACY_SPACING, weights=ALL, sign_scale=3.0)
    s = _t(sdf).cuda()
    runs = []
    for _ in range(5):
        loss, grad = lr.value_and_grad(s)
        assert loss.is_cuda and loss.dtype == torch.float32 and loss.dim() == 0 and grad.is_cuda and grad.shape == s.shape and not grad.requires_grad
        assert lr.terms.shape == (3,) and lr.terms.dtype == torch.float32 and lr.num_crossings.shape == (1,) and lr.num_crossings.dtype == torch.int32
        runs.append(tuple(_bits(_np(a)) for a in (loss, lr.terms, lr.num_crossings, grad)))
    assert all(r == runs[0] for r in runs)
    value = lr.value(s)
    assert (_bits(_np(value)), _bits(_np(lr.terms)), _bits(_np(lr.num_crossings))) == runs[0][:3]


def test_autograd_equals_value_and_grad(psdr):
    import torch
    shape, sdf = _case(seed=52)
    lr = psdr.LatticeRegularizer(shape, ref.ACCURACY_SPACING, weights=ALL, sign_scale=3.0)
    loss, grad = lr.value_and_grad(_t(sdf))
    assert np.abs(_np(grad)).max() > 0
    s = _t(sdf).cuda().requires_grad_()
    out = lr(s)
    assert out.is_cuda and out.dim() == 0 and torch.equal(out.detach(), loss)
    out.backward()
    assert torch.equal(s.grad, grad)
    s.grad = None
    (3.0 * lr(s)).backward()
    assert torch.equal(s.grad, 3.0 * grad)
    # a float64 sdf on the host: the gradient returns to its device and dtype
    h = _t(sdf.astype(np.float64)).requires_grad_()
    lr(h).backward()
    assert h.grad.dtype == torch.float64 and not h.grad.is_cuda and torch.equal(h.grad, grad.cpu().double())
    # the attributes are read at every call
    lr.weights = SINGLE["eikonal"]
    assert _bits(_np(lr.value_and_grad(_t(sdf))[1])) == _bits(_eval(psdr, shape, ref.ACCURACY_SPACING, SINGLE["eikonal"], 1.0, sdf)[2])


@pytest.mark.parametrize("form", ("S", "default"))
def test_streams(psdr, form):
    """both forms of the delayed producer; sdf rolled along its first axis is the decoy"""
    import torch
    shape, sdf = _case(seed=53)
    lr = psdr.LatticeRegularizer(shape, ref.ACCURACY_SPACING, weights=ALL, sign_scale=3.0)
    ss = Slot(torch, sdf)
    fetch = lambda out: tuple(_np(a) for a in out)

    def call():
        loss, grad = lr.value_and_grad(ss.buf)
        return (loss, lr.terms, lr.num_crossings, grad)
    base = run_plain(torch, [ss], call, fetch)
    decoy = lr.value_and_grad(ss._decoy)
    assert _bits(_np(decoy[0])) != _bits(base[0]) and _bits(_np(decoy[1])) != _bits(base[3])          # the decoy is told apart
    S = torch.cuda.Stream()

    # autograd under the stream first (backward waits on the host for the engine's thread, and the first launch on a new stream takes milliseconds: no self-check)
    def autograd():
        s = ss.buf.clone().requires_grad_()
        lr(s).backward()
        return (s.grad,)
    got = run_on_stream(torch, S, form, [ss], autograd, fetch, returns_early=False)
    assert _bits(got[0]) == _bits(base[3])
    # the Python layer returns without a synchronisation: the delay is still running when it does
    got = run_on_stream(torch, S, form, [ss], call, fetch)
    assert all(_bits(a) == _bits(b) for a, b in zip(got, base))
    got = run_on_stream(torch, S, form, [ss], lambda: (lr.value(ss.buf),), fetch)
    assert _bits(got[0]) == _bits(base[0])


# ---- 5. one DMTet step

def test_one_dmtet_step_reaches_every_lattice_vertex(psdr):
    """marching tetrahedra alone leaves every vertex that is no end of a crossing edge exactly zero; with the regulariser those vertices move too"""
    import torch
    shape = (9, 9, 9)
    pos = psdr.lattice_points(shape, -1.0, 1.0)
    sdf0 = (np.linalg.norm(pos.numpy().astype(np.float64) - np.array([0.03, -0.02, 0.05]), axis=1) - 0.61).astype(np.float32)
    assert np.abs(sdf0).min() >= 1e-4
    m = ref.crossing_counts(sdf0, shape).ravel()
    far = m == 0
    assert far.sum() > 100 and (~far).sum() > 100
    mt = psdr.MarchingTetrahedra(shape)
    lr = psdr.LatticeRegularizer(shape, psdr.lattice_spacing(shape, -1.0, 1.0), weights=(1.0, 0.1, 0.1), sign_scale=10.0)
    alone = _t(sdf0).cuda().requires_grad_()
    mt.extract(alone)
    mt(alone, pos).square().sum().backward()
    assert not _np(alone.grad)[far].any() and _np(alone.grad)[~far].any()
    sdf = _t(sdf0).cuda().requires_grad_()
    mt.extract(sdf)
    (lr(sdf) + mt(sdf, pos).square().sum()).backward()
    g = _np(sdf.grad)
    assert np.isfinite(g).all() and (g[far] != 0).sum() > 0.9 * far.sum()
    assert int(_np(lr.num_crossings)[0]) == mt.topology.num_vertices
    print("one DMTet step: %d of %d vertices far from any crossing receive a gradient, max |grad| there %.3g" % ((g[far] != 0).sum(), far.sum(), np.abs(g[far]).max()))
