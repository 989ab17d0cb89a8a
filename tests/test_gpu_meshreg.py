"""GPU tests of the mesh regularisers (psdr_jit_amd/meshreg.py, csrc/hip/meshreg.hip) against the float64 checker tests/meshreg_ref.py.

The accuracy rule, per case, per term, for the value and for the gradient: e_gpu <= 4 max(e_32, u G), with e_gpu = max |device - float64|, e_32 = max |float32 checker -
float64|, G = max |float64|, u = 2^-24 (meshreg_ref.py says why).  Cases: one vertex and no face (everything exactly 0); one triangle; two triangles at a generic fold;
TETRAHEDRON, BOWTIE, BOOK; fan(5); fan(70) (a hub above one wave, an unused vertex); grid(3); grid(17) (289 vertices and 1825 elements cross a 256-lane workgroup);
grid(27); the bunny; and a mesh with two zero-area faces and a zero-length edge.  Each with all three weights on (1, 0.5, 2: the loss, the three terms and the whole
gradient), each term alone, and target_length 0 and 0.05.  Every test prints the worst e_gpu / max(e_32, u G) it saw per term.

Measured on an MI355X, the worst ratio over all cases: values - laplacian 1.24 (bunny), normal 1.66 (fan5), edge 2.45 (bowtie, L0 = 0.05), loss 2.45;
gradients - laplacian 1.00, normal 1.42 (fold), edge 1.85 (bunny, L0 = 0.05), all on 1.55 (fan5, L0 = 0.05).  The folded hinge gave 2 - 3.6e-7.

Then the defined edge cases (a flat hinge, a folded one, a term switched off), repeatability, the value-only call, autograd alone and through Subdivision and the
Laplacian preconditioner, and both stream forms of tests/stream_cases.py."""
import ctypes as C

import numpy as np
import pytest

import meshreg_ref as ref
import subdiv_ref as sref
from stream_cases import Slot, run_on_stream, run_plain

pytestmark = pytest.mark.gpu

ALL_ON = (1.0, 0.5, 2.0)
ALONE = {"laplacian": (1.0, 0.0, 0.0), "normal": (0.0, 1.0, 0.0), "edge": (0.0, 0.0, 1.0)}


@pytest.fixture(scope="module")
def psdr():
    import __graft_entry__
    __graft_entry__.build()
    import psdr_jit_amd
    return psdr_jit_amd


def _call(reg, v, weights, L0):
    """-> (loss, terms [3], grad [n, 3]) as numpy"""
    import torch
    reg.weights, reg.target_length = weights, L0
    loss, grad = reg.value_and_grad(torch.from_numpy(np.ascontiguousarray(v)))
    return float(loss.cpu()), reg.terms.cpu().numpy(), grad.cpu().numpy()


def _held(what, worst, key, dev, f32, f64):
    r, e_gpu, e_32, G = ref.ratio(dev, f32, f64)
    worst[key] = max(worst.get(key, 0.0), r)
    assert np.isfinite(np.asarray(dev)).all(), what
    assert r <= 4.0, "%s: e_gpu = %.3g, e_32 = %.3g, u G = %.3g: ratio %.3g > 4" % (what, e_gpu, e_32, ref.U * G, r)


@pytest.mark.parametrize("L0", [0.0, 0.05])
@pytest.mark.parametrize("name", ref.CASES + ("degenerate",))
def test_accuracy_rule(psdr, name, L0):
    faces, n, v = ref.case(name)
    f64, f32, topo = ref.reference(name, L0)
    reg = psdr.MeshRegularizer(np.array(faces, np.int64).reshape(-1, 3), n)
    assert len(reg.topology.edges) == len(topo["edges"]) and len(reg.topology.hinges) == len(topo["hinges"])
    worst = {}
    for k, term in enumerate(ref.TERMS):
        loss, terms, grad = _call(reg, v, ALONE[term], L0)
        what = "%s, L0 = %g, %s alone" % (name, L0, term)
        _held(what + ": value", worst, term + " value", terms[k], f32[term][0], f64[term][0])
        _held(what + ": gradient", worst, term + " gradient", grad, f32[term][1], f64[term][1])
        assert loss == terms[k] and all(terms[j] == 0 for j in range(3) if j != k), what
    loss, terms, grad = _call(reg, v, ALL_ON, L0)
    what = "%s, L0 = %g, all on" % (name, L0)
    for k, term in enumerate(ref.TERMS):
        _held(what + ": " + term, worst, term + " value", terms[k], f32[term][0], f64[term][0])
    l64, g64 = ref.combine(f64, ALL_ON)
    l32, g32 = ref.combine(f32, ALL_ON, np.float32)
    _held(what + ": loss", worst, "loss", loss, l32, l64)
    _held(what + ": gradient", worst, "gradient", grad, g32, g64)
    if name == "point":
        assert loss == 0 and not terms.any() and not grad.any()
    print("%s, L0 = %g: worst e_gpu / max(e_32, u G): %s" % (name, L0, ", ".join("%s %.2f" % kv for kv in sorted(worst.items()))))


def test_flat_hinge(psdr):
    """an exactly flat hinge: the normal term is at most 4 u and finite, and so is its gradient"""
    u = ref.U
    # in the plane z = 0, c left of the edge and d right of it: both normals are exactly (0, 0, |n|)
    flat = np.array([[0.1, -0.7, 0], [0.3, 0.9, 0], [-0.8, 0.2, 0], [0.7, -0.1, 0]], np.float32)
    tilted = np.array([[0, 0, 0], [4, 1, 6], [1, 3, 7], [3, -2, -1]], np.float32) / 8.0          # in the plane z = x + 2 y: the cross products are exact
    for v in (flat, tilted):
        reg = psdr.MeshRegularizer(np.array([[0, 1, 2], [1, 0, 3]]), 4)
        loss, terms, grad = _call(reg, v, ALONE["normal"], 0.0)
        f64 = ref.evaluate(v, [[0, 1, 2], [1, 0, 3]], 4)
        assert f64["normal"][0] <= 1e-30
        assert np.isfinite(terms).all() and np.isfinite(grad).all() and 0 <= terms[1] <= 4 * u and loss == terms[1]
        scale = 1.0 / min(np.linalg.norm(np.cross(v[1] - v[0], v[2] - v[0])), np.linalg.norm(np.cross(v[3] - v[0], v[1] - v[0])))
        # |d / dn| <= |w| / |n| with |w| <= 6 u (two unit vectors, each component rounded three times); a corner sums at most four lever arms, each shorter than 2
        assert np.abs(grad).max() <= 48 * u * scale


def test_folded_hinge(psdr):
    """a hinge folded back onto itself (d sits on c): the normal term is 2 within 8 u, the gradient finite"""
    v = ref._uniform(4, 22)
    v[3] = v[2]
    reg = psdr.MeshRegularizer(np.array([[0, 1, 2], [1, 0, 3]]), 4)
    loss, terms, grad = _call(reg, v, ALONE["normal"], 0.0)
    assert abs(float(terms[1]) - 2.0) <= 8 * ref.U and loss == terms[1]
    assert np.isfinite(grad).all()
    f64, f32 = ref.evaluate(v, [[0, 1, 2], [1, 0, 3]], 4), ref.evaluate(v, [[0, 1, 2], [1, 0, 3]], 4, dtype=np.float32)
    assert abs(f64["normal"][0] - 2.0) <= 1e-15
    print("folded hinge: value - 2 = %.3g, largest gradient entry %.3g (float64: %.3g, float32 checker: %.3g)" %
          (float(terms[1]) - 2.0, np.abs(grad).max(), np.abs(f64["normal"][1]).max(), np.abs(f32["normal"][1]).max()))


@pytest.mark.parametrize("name", ["grid17", "fan70", "degenerate"])
def test_a_term_of_weight_zero_is_left_out(psdr, name):
    """its value is exactly 0 and the gradient is the other terms' bit for bit: the terms' scaled gradients are added in the order laplacian, normal, edge, those that
    are off left out - so the float32 sum of the single-term gradients IS the gradient - and target_length is not read when the edge term is off"""
    faces, n, v = ref.case(name)
    reg = psdr.MeshRegularizer(np.array(faces), n)
    w = (0.75, 1.5, 0.3)
    single = [_call(reg, v, tuple(w[j] if j == k else 0.0 for j in range(3)), 0.05) for k in range(3)]
    for k in range(3):
        assert single[k][1][k] > 0 and all(single[k][1][j] == 0 for j in range(3) if j != k) and np.abs(single[k][2]).max() > 0
    for off in range(3):
        on = [k for k in range(3) if k != off]
        loss, terms, grad = _call(reg, v, tuple(0.0 if j == off else w[j] for j in range(3)), 0.05)
        assert terms[off] == 0 and all(terms[k] == single[k][1][k] for k in on)
        want = single[on[0]][2] + single[on[1]][2]
        assert want.dtype == np.float32 and grad.tobytes() == want.tobytes()
        assert np.float32(loss) == np.float32(single[on[0]][0]) + np.float32(single[on[1]][0])
    loss, terms, grad = _call(reg, v, w, 0.05)
    assert grad.tobytes() == ((single[0][2] + single[1][2]) + single[2][2]).tobytes()
    a, b = _call(reg, v, (w[0], w[1], 0.0), 0.0), _call(reg, v, (w[0], w[1], 0.0), 0.7)
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    loss, terms, grad = _call(reg, v, (0.0, 0.0, 0.0), 0.05)
    assert loss == 0 and not terms.any() and not grad.any()


def test_five_calls_return_identical_bits(psdr):
    import torch
    faces, n, v = ref.bunny()
    reg = psdr.MeshRegularizer(np.array(faces), n, weights=ALL_ON, target_length=0.05)
    vd = torch.from_numpy(v).cuda()
    runs = []
    for _ in range(5):
        loss, grad = reg.value_and_grad(vd)
        runs.append((loss.cpu().numpy().tobytes(), reg.terms.cpu().numpy().tobytes(), grad.cpu().numpy().tobytes()))
    assert all(r == runs[0] for r in runs[1:])
    # another handle of the same mesh as well
    other = psdr.MeshRegularizer(np.array(faces), n, weights=ALL_ON, target_length=0.05)
    loss, grad = other.value_and_grad(vd)
    assert (loss.cpu().numpy().tobytes(), other.terms.cpu().numpy().tobytes(), grad.cpu().numpy().tobytes()) == runs[0]


def _raw_eval(reg, vd, weights, L0, want_grad):
    import torch
    from psdr_jit_amd import cabi
    out = torch.full((4,), float("nan"), device="cuda")
    grad = torch.full_like(vd, float("nan")) if want_grad else None
    cabi.check(cabi.lib().psdr_hip_meshreg_eval(reg._handle.ptr, vd.data_ptr(), (C.c_float * 3)(*weights), L0, out.data_ptr(), grad.data_ptr() if want_grad else None,
                                                int(torch.cuda.current_stream().cuda_stream)))
    return out, grad


def test_value_only_call(psdr):
    """grad NULL through the C ABI: the same out bits, and out = (loss, terms)"""
    import torch
    faces, n, v = ref.bunny()
    reg = psdr.MeshRegularizer(np.array(faces), n)
    vd = torch.from_numpy(v).cuda()
    for weights, L0 in ((ALL_ON, 0.05), (ALL_ON, 0.0), (ALONE["normal"], 0.0)):
        full, grad = _raw_eval(reg, vd, weights, L0, True)
        only, _none = _raw_eval(reg, vd, weights, L0, False)
        assert full.cpu().numpy().tobytes() == only.cpu().numpy().tobytes() and np.isfinite(full.cpu().numpy()).all() and np.isfinite(grad.cpu().numpy()).all()
        loss, terms, g = _call(reg, v, weights, L0)
        assert np.float32(loss) == full[0].item() and terms.tobytes() == full[1:].cpu().numpy().tobytes() and g.tobytes() == grad.cpu().numpy().tobytes()


def test_autograd_scales_the_forward_gradient(psdr):
    import torch
    faces, n, v = ref.case("grid17")
    reg = psdr.MeshRegularizer(np.array(faces), n, weights=ALL_ON, target_length=0.05)
    loss, grad = reg.value_and_grad(torch.from_numpy(v))
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda and not loss.requires_grad and not grad.requires_grad and reg.terms.shape == (3,)
    leaf = torch.from_numpy(v).cuda().requires_grad_()
    out = reg(leaf)
    assert out.dim() == 0 and out.dtype == torch.float32 and out.is_cuda and out.item() == loss.item() and not reg.terms.requires_grad
    (3 * out).backward()
    assert torch.equal(leaf.grad, 3 * grad)
    # v on the host in float64: the gradient returns to its device and dtype
    host = torch.from_numpy(v.astype(np.float64)).requires_grad_()
    (3 * reg(host)).backward()
    assert host.grad.dtype == torch.float64 and not host.grad.is_cuda and torch.equal(host.grad, (3 * grad).cpu().double())
    # a schedule changes the plain attributes between calls
    reg.weights = (0.0, 0.0, 1.0)
    reg.target_length = 0.0
    assert reg(leaf).item() == reg.terms[2].item() and reg.terms[0].item() == 0
    for bad in ((1.0, -1.0, 0.0), (1.0, 1.0)):
        reg.weights = bad
        with pytest.raises(ValueError):
            reg(leaf)
    reg.weights = ALL_ON
    for bad in (torch.zeros(n, 2), torch.zeros(n + 1, 3), torch.zeros(n, 3, dtype=torch.int32)):
        with pytest.raises(ValueError):
            reg(bad)


def test_autograd_through_subdivision(psdr):
    """on grid(5) with one Loop level the gradient of reg(sub.refine(c)) with respect to c equals sub.restrict(grad) exactly"""
    import torch
    faces, n, c0 = ref.case("grid5")
    sub = psdr.Subdivision(np.array(faces), n, levels=1)
    reg = psdr.MeshRegularizer(sub.faces, sub.num_vertices_out, weights=ALL_ON, target_length=0.05)
    c = torch.from_numpy(c0).cuda().requires_grad_()
    reg(sub.refine(c)).backward()
    _loss, grad = reg.value_and_grad(sub.refine(c.detach()))
    assert grad.abs().max() > 0 and torch.equal(c.grad, sub.restrict(grad))


def test_autograd_through_the_preconditioner(psdr):
    """on grid(9) the gradient of reg(pre.from_differential(u)) matches pre.from_differential applied to grad within the solve's rtol: M^-1 has norm at most 1, so two
    solves of M x = grad that each leave a residual of at most rtol |grad| differ by at most 2 rtol |grad|"""
    import torch
    faces, n, v0 = ref.case("grid9")
    pre = psdr.LaplacianPreconditioner(np.array(faces), n)
    reg = psdr.MeshRegularizer(np.array(faces), n, weights=ALL_ON, target_length=0.05)
    u = pre.to_differential(torch.from_numpy(v0)).detach().requires_grad_()
    reg(pre.from_differential(u)).backward()
    _loss, grad = reg.value_and_grad(pre.from_differential(u.detach()))
    want = pre.from_differential(grad)
    assert grad.norm() > 0 and (u.grad - want).norm().item() <= 2 * pre.rtol * grad.norm().item()


@pytest.mark.parametrize("form", ("S", "default"))
def test_streams(psdr, form):
    """both forms of the delayed producer: the vertex array rolled along its first axis is the decoy"""
    import torch
    import stream_cases as sc_
    faces, n, v = ref.bunny()
    reg = psdr.MeshRegularizer(np.array(faces), n, weights=ALL_ON, target_length=0.05)
    slot = Slot(torch, v)
    fetch = lambda t: tuple(x.cpu().numpy() for x in t)
    call = lambda: reg.value_and_grad(slot.buf) + (reg.terms,)
    base = run_plain(torch, [slot], call, fetch)
    decoy = _call(reg, sc_.decoy_of(v), ALL_ON, 0.05)
    assert abs(decoy[0] - float(base[0])) > 1e-3 * abs(float(base[0]))          # (the decoy is told apart)
    S = torch.cuda.Stream()

    # autograd under the stream first (backward waits on the host for the engine's thread, and the first launch on a new stream takes milliseconds: no self-check)
    def autograd():
        leaf = slot.buf.clone().requires_grad_()
        reg(leaf).backward()
        return (leaf.grad,)
    assert run_on_stream(torch, S, form, [slot], autograd, fetch, returns_early=False)[0].tobytes() == base[1].tobytes()
    # the Python layer returns without a synchronisation: the delay is still running when it does
    got = run_on_stream(torch, S, form, [slot], call, fetch)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, base))
    # and so does the C ABI called directly
    raw = run_on_stream(torch, S, form, [slot], lambda: _raw_eval(reg, slot.buf, ALL_ON, 0.05, True), fetch)
    assert raw[0][0] == base[0] and raw[0][1:].tobytes() == base[2].tobytes() and raw[1].tobytes() == base[1].tobytes()
