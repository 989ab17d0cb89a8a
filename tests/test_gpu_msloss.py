"""GPU tests of the multi-scale image loss (psdr_jit_amd/msloss.py, csrc/hip/msloss.hip) against the float64 checker tests/msloss_ref.py: the residual pyramid bit for
bit on exact inputs, loss, level losses and gradient within a derived bound for both norms, with and without weights, truncated and weighted levels, repeatability,
handle state, autograd (down to the parameter of a rendered scene), streams and every refusal that needs a real handle.

The bound is derived, not tuned.  u = 2^-24, gamma_m = m u / (1 - m u); a float32 sum of n terms in any order errs by at most gamma_{n-1} sum |t|.
  pyramid   d_0 = fl(w fl(img - target)) is 2 roundings, a level 3 more ((a + b) + (c + d), the divisor is a power of two):
            |d_l - d64_l| <= gamma_{3l+2} (the level-l mean of |d_0| over the pixel's footprint)
  level     the kernels add the n = C W_l H_l values rho(d_l) in a fixed order (n - 1 roundings, whatever the order), rho = d d is one rounding, 1 / n is rounded
            once and multiplied once; with d_l's own 3l + 2 that is at most n + 3l + 4:   |level_loss_l - want| <= gamma_{n+3l+4} sum |rho(d_l)| / n.
            n is kept as the issue states it: the reduction's depth (a lane's <= 12 elements, 6 shuffle steps, 4 waves, the tiles' partials) would only tighten it.
  loss      sum_l fl(lambda_l level_loss_l) from 0: one product and at most L additions on top of the levels' errors B_l:
            |loss - want| <= sum |lambda_l| B_l + gamma_{L+1} sum |lambda_l| (level_loss_l + B_l)
  gradient  G_l = fl(coef_l rho'(d_l)) + G_{l+1} / count: coef_l = lambda_l / n_l is rounded twice (double, then float), the product once (rho' = +-1, 0 or 2 d
            is exact), at most L - 1 additions, the divisions by 1, 2, 4 are exact, the weight one more: L + 3, and with d_l's 3l + 2 at most 4L + 6:
            |grad - want| <= gamma_{4L+6} sum_l |term_l|,  term_l = weight P_1^T .. P_l^T coef_l rho'(d_l) in float64.
On exact inputs (k / 2^b with b + 2 (L - 1) <= 21: every d_l is a float32, which the test asserts on the CPU first) the pyramid is compared bit for bit and the l1
signs are those of the checker, zeros included.  On Gaussian inputs l2 is held to the same bounds; l1, whose rho' jumps at 0, is compared with the checker evaluated on
the device's own pyramid: each stage is fed the previous stage's device output, no sign can flip, no pixel is left out.

Shapes (W x H): 1 x 1 a single pixel; 9 x 1 a single row; 32 x 32 exactly one tile; 33 x 33 one-pixel partial tiles, odd at levels 0 .. 3; 37 x 19; 70 x 45 3 x 2 tiles and an
odd coarse image; 64 x 96 exact tiles; 257 x 130 ten levels, a 9 x 5 level-5 image that the one-workgroup kernel takes over."""
import ctypes as C

import numpy as np
import pytest

import msloss_ref as ref
from stream_cases import Slot, run_on_stream, run_plain

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SHAPES = [(1, 1), (9, 1), (32, 32), (33, 33), (37, 19), (70, 45), (64, 96), (257, 130)]
CASES = [(W, H, 3) for W, H in SHAPES] + [(33, 33, 1), (33, 33, 4), (70, 45, 1), (70, 45, 4)]
NORMS = ("l1", "l2")


@pytest.fixture(scope="module")
def psdr():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists)")
    import __graft_entry__
    __graft_entry__.build()
    import psdr_jit_amd
    return psdr_jit_amd


def gamma(m):
    m = np.asarray(m, np.float64)
    return m * U / (1.0 - m * U)


def _exact_inputs(W, H, Cn, seed=0):
    """img, target, a one-channel mask with zeros, a C-channel weight: multiples of 2^-b of magnitude <= 2 with b + 2 (L - 1) <= 21 for the residual (the weights
    have one fractional bit, the images b - 1); about one value in eight of img equals target's, so d_0 holds exact zeros"""
    L = len(ref.shapes(W, H))
    b = max(1, min(9, 21 - 2 * (L - 1) - 1))
    assert (b + 1) + 2 * (L - 1) <= 21
    rng = np.random.default_rng([seed, W, H, Cn])
    n = W * H
    q = float(2 ** b)
    img = rng.integers(-2 * q, 2 * q + 1, (n, Cn)) / q
    tgt = rng.integers(-2 * q, 2 * q + 1, (n, Cn)) / q
    same = rng.random((n, Cn)) < 0.125
    tgt[same] = img[same]
    mask = (rng.random((n, 1)) < 0.75).astype(np.float64)
    wc = rng.integers(0, 5, (n, Cn)) / 2.0
    img, tgt, mask, wc = (a.astype(np.float32) for a in (img, tgt, mask, wc))
    for w in (None, mask, wc):
        p32, p64 = ref.pyramid(img, tgt, W, H, w, dtype=np.float32), ref.pyramid(img, tgt, W, H, w)
        assert all(a.dtype == np.float32 and np.array_equal(a.astype(np.float64), d) for a, d in zip(p32, p64)), "the test's inputs are not exact in float32"
    return img, tgt, mask, wc


def _gauss_inputs(W, H, Cn, seed=1):
    rng = np.random.default_rng([seed, W, H, Cn])
    n = W * H
    return (rng.standard_normal((n, Cn)).astype(np.float32), rng.standard_normal((n, Cn)).astype(np.float32),
            (0.25 + rng.random((n, 1))).astype(np.float32), (0.25 + rng.random((n, Cn))).astype(np.float32))


def _run(psdr, ms, img, tgt, weight):
    """(loss, level losses, gradient, pyramid) of the device, as numpy"""
    import torch
    t = lambda a: None if a is None else torch.from_numpy(a).cuda()
    loss, grad = ms.value_and_grad(t(img), t(tgt), t(weight))
    assert loss.is_cuda and loss.dim() == 0 and loss.dtype == torch.float32 and tuple(grad.shape) == img.shape
    pyr = ms.residual_pyramid()
    assert [tuple(d.shape) for d in pyr] == [(w * h, ms.channels) for w, h in ms.shapes]
    return float(loss.cpu()), ms.level_losses.cpu().numpy().astype(np.float64), grad.cpu().numpy(), [d.cpu().numpy() for d in pyr]


def _check_values(label, got, pyr64, W, H, norm, weight, lam):
    """loss, level losses and gradient of the device against the checker on `pyr64`, within the module docstring's bounds, every entry"""
    loss, ll, grad, _pyr = got
    L = len(pyr64)
    lam = np.ones(L) if lam is None else np.asarray(np.float32(lam), np.float64)
    want_loss, want_ll = ref.losses(pyr64, norm, lam)
    n = np.array([d.size for d in pyr64], np.float64)
    B = gamma(n + 3 * np.arange(L) + 4) * want_ll
    err = np.abs(ll - want_ll)
    print(label, "level losses: worst error / bound %.3f" % float((err / np.maximum(B, 1e-300)).max()))
    assert np.isfinite(ll).all() and np.all(err <= B), (label, err, B)
    B_loss = float((np.abs(lam) * B).sum() + gamma(L + 1) * (np.abs(lam) * (want_ll + B)).sum())
    print(label, "loss %.9g want %.9g: error / bound %.3f" % (loss, want_loss, abs(loss - want_loss) / max(B_loss, 1e-300)))
    assert np.isfinite(loss) and abs(loss - want_loss) <= B_loss, (label, loss, want_loss, B_loss)
    terms = ref.gradient_terms(pyr64, W, H, norm, weight, lam)
    want, bound = sum(terms), gamma(4 * L + 6) * sum(np.abs(t) for t in terms)
    err = np.abs(grad.astype(np.float64) - want)
    print(label, "gradient: worst error / bound %.3f, max |want| %.3g" % (float((err / np.maximum(bound, 1e-300)).max()), float(np.abs(want).max())))
    assert np.isfinite(grad).all() and np.all(err <= bound), label
    return want


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("W,H,Cn", CASES)
def test_exact_inputs(psdr, W, H, Cn, norm):
    img, tgt, mask, wc = _exact_inputs(W, H, Cn)
    ms = psdr.MultiScaleLoss(W, H, channels=Cn, norm=norm)
    assert ms.shapes == ref.shapes(W, H) == psdr.pyramid_shapes(W, H) and ms.levels == len(ms.shapes)
    for name, weight in (("none", None), ("mask", mask), ("mask flat", mask), ("C-channel", wc)):
        label = "%dx%d C=%d %s weight %s" % (W, H, Cn, norm, name)
        pyr64 = ref.pyramid(img, tgt, W, H, weight)
        got = _run(psdr, ms, img, tgt, weight.reshape(-1) if name == "mask flat" else weight)
        for l, (a, d) in enumerate(zip(got[3], pyr64)):
            assert a.dtype == np.float32 and np.array_equal(a.astype(np.float64), d), (label, "level", l)
        assert any((d == 0).any() for d in pyr64) or W * H * Cn < 64          # sign(0) = 0 is exercised
        _check_values(label, got, pyr64, W, H, norm, weight, None)
        if norm == "l1" and name == "mask" and W * H >= 64:
            # where the mask is 0 every term is: the bound is 0 there and the gradient exactly 0 (asserted above); such pixels exist
            assert np.all(got[2][mask.reshape(-1) == 0] == 0.0) and (mask == 0).any()


@pytest.mark.parametrize("norm", NORMS)
def test_truncated_and_weighted_levels(psdr, norm):
    import torch
    W, H, Cn = 70, 45, 3
    img, tgt, mask, wc = _exact_inputs(W, H, Cn)
    full = len(ref.shapes(W, H))
    for levels, lam in ((3, None), (4, (1.0, 0.5, 0.0, 2.0)), (6, None), (7, None), (full, tuple(0.25 * (k % 5) for k in range(full)))):
        ms = psdr.MultiScaleLoss(W, H, channels=Cn, levels=levels, norm=norm, level_weights=lam)
        assert ms.levels == levels == len(ms.shapes)
        for weight in (None, wc):
            pyr64 = ref.pyramid(img, tgt, W, H, weight, levels)
            got = _run(psdr, ms, img, tgt, weight)
            assert len(got[3]) == levels and all(np.array_equal(a.astype(np.float64), d) for a, d in zip(got[3], pyr64))
            _check_values("70x45 levels=%d lambda=%s %s" % (levels, lam, norm), got, pyr64, W, H, norm, weight, lam)
    # img == target: loss 0 and gradient 0, exactly
    ms = psdr.MultiScaleLoss(W, H, channels=Cn, norm=norm)
    loss, ll, grad, pyr = _run(psdr, ms, img, img.copy(), wc)
    assert loss == 0.0 and not ll.any() and not grad.any() and not any(d.any() for d in pyr)
    x = torch.from_numpy(img).cuda().requires_grad_()
    out = ms(x, torch.from_numpy(img).cuda())
    out.backward()
    assert float(out.detach()) == 0.0 and not x.grad.any()


@pytest.mark.parametrize("W,H,Cn", [(33, 33, 3), (70, 45, 4), (257, 130, 3), (9, 1, 1)])
def test_gaussian_inputs(psdr, W, H, Cn):
    img, tgt, w1, wc = _gauss_inputs(W, H, Cn)
    for norm in NORMS:
        ms = psdr.MultiScaleLoss(W, H, channels=Cn, norm=norm)
        for name, weight in (("none", None), ("one channel", w1), ("C-channel", wc)):
            label = "%dx%d C=%d %s gaussian, weight %s" % (W, H, Cn, norm, name)
            pyr64 = ref.pyramid(img, tgt, W, H, weight)
            foot = ref.footprint_mean_abs(img, tgt, W, H, weight)
            got = _run(psdr, ms, img, tgt, weight)
            worst = 0.0
            for l, (a, d, f) in enumerate(zip(got[3], pyr64, foot)):
                err, bound = np.abs(a.astype(np.float64) - d), gamma(3 * l + 2) * f
                worst = max(worst, float((err / bound).max()))
                assert np.isfinite(a).all() and np.all(err <= bound), (label, "level", l)
            print(label, "pyramid: worst error / bound %.3f" % worst)
            if norm == "l2":
                _check_values(label, got, pyr64, W, H, norm, weight, None)
            else:
                _check_values(label + " (on the device's pyramid)", got, [a.astype(np.float64) for a in got[3]], W, H, norm, weight, None)


def test_same_bits_every_call_and_no_state_left(psdr):
    import torch
    W, H, Cn = 70, 45, 3
    a_img, a_tgt, a_w1, a_wc = (torch.from_numpy(x).cuda() for x in _gauss_inputs(W, H, Cn, seed=2))
    b_img, b_tgt, _b1, _bc = (torch.from_numpy(x).cuda() for x in _gauss_inputs(W, H, Cn, seed=3))
    for norm in NORMS:
        ms = psdr.MultiScaleLoss(W, H, channels=Cn, norm=norm)
        la, ga = ms.value_and_grad(a_img, a_tgt, a_wc)
        lla, pa = ms.level_losses, ms.residual_pyramid()
        lb, gb = ms.value_and_grad(b_img, b_tgt)                      # another pair, no weight, on the same handle
        assert not torch.equal(la, lb) and not torch.equal(ga, gb)
        la2, ga2 = ms.value_and_grad(a_img, a_tgt, a_wc)
        assert torch.equal(la, la2) and torch.equal(ga, ga2) and torch.equal(lla, ms.level_losses)
        assert all(torch.equal(p, q) for p, q in zip(pa, ms.residual_pyramid()))
        fresh = psdr.MultiScaleLoss(W, H, channels=Cn, norm=norm)
        lf, gf = fresh.value_and_grad(a_img, a_tgt, a_wc)
        assert torch.equal(la, lf) and torch.equal(ga, gf)
        # grad = NULL: the same loss bits, and the pyramid of that call
        out, none = ms._eval(b_img, b_tgt, None, False)
        assert none is None and torch.equal(out[0], lb)
        out, none = ms._eval(a_img, a_tgt, a_wc, False)
        assert torch.equal(out[0], la) and torch.equal(out[1:], lla) and all(torch.equal(p, q) for p, q in zip(pa, ms.residual_pyramid()))


def test_autograd(psdr):
    import torch
    W, H, Cn = 37, 19, 3
    img, tgt, w1, _wc = (torch.from_numpy(x).cuda() for x in _gauss_inputs(W, H, Cn, seed=4))
    for norm in NORMS:
        ms = psdr.MultiScaleLoss(W, H, channels=Cn, norm=norm)
        _loss, g = ms.value_and_grad(img, tgt, w1)
        x, t, w = img.clone().requires_grad_(), tgt.clone().requires_grad_(), w1.clone().requires_grad_()
        out = ms(x, t, w)
        assert out.dim() == 0 and out.requires_grad and not ms.level_losses.requires_grad and tuple(ms.level_losses.shape) == (ms.levels,)
        out.backward()
        assert torch.equal(x.grad, g) and torch.equal(t.grad, -g) and w.grad is None and float(g.abs().max()) > 0
        x2 = img.clone().requires_grad_()
        (3.0 * ms(x2, tgt, w1)).backward()
        assert torch.equal(x2.grad, 3.0 * g)
        # only the target asks for a gradient; a CPU float64 leaf gets a CPU float64 gradient
        t64 = tgt.cpu().double().requires_grad_()
        ms(img, t64, w1).backward()
        assert t64.grad.device.type == "cpu" and t64.grad.dtype == torch.float64 and torch.equal(t64.grad, (-g).cpu().double())


def test_gradient_reaches_the_scene_parameter(psdr):
    """the README box at 32 x 32 and 2 spp: P.grad through ms equals P.grad of <g, renderD> with g the fused image gradient, bit for bit - the reverse sweep is
    deterministic and backward hands it g times exactly 1"""
    import torch
    import test_gpu_api as api
    grads = []
    for use_ms in (True, False):
        P = psdr.FloatD(0.).requires_grad_()
        sc = api._readme_scene(psdr, P, res=32, spp=2)
        integ = psdr.PathTracer(2)
        ms = psdr.MultiScaleLoss(32, 32)
        if not grads:
            target = 0.5 * integ.renderC(sc, 0, seed=3)
        img = integ.renderD(sc, 0, seed=11)
        if use_ms:
            ms(img, target).backward()
        else:
            _loss, g = ms.value_and_grad(img.detach(), target)
            (g.detach() * img).sum().backward()
        grads.append(P.grad.detach().cpu().clone())
    print("P.grad", float(grads[0]), float(grads[1]))
    assert torch.equal(grads[0], grads[1]) and float(grads[0]) != 0.0 and np.isfinite(float(grads[0]))


@pytest.mark.parametrize("form", ("S", "default"))
def test_made_on_one_stream_evaluated_on_another(psdr, form):
    import torch
    from psdr_jit_amd import cabi
    import stream_cases as sc_
    W, H, Cn, norm = 70, 45, 3, "l2"
    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    img_np, tgt_np, _w1, wc_np = _gauss_inputs(W, H, Cn, seed=5)
    img, tgt = Slot(torch, img_np), Slot(torch, tgt_np)
    wc = torch.from_numpy(wc_np).cuda()
    plain = psdr.MultiScaleLoss(W, H, channels=Cn, norm=norm)
    fetch = lambda o: [t.cpu().numpy() for t in o]
    base = run_plain(torch, [img, tgt], lambda: plain.value_and_grad(img.buf, tgt.buf, wc) + (plain.level_losses,), fetch)
    for s in (img, tgt):
        s.reset()
    torch.cuda.synchronize()
    with torch.cuda.stream(A):
        sc_.delay(torch)
        ms = psdr.MultiScaleLoss(W, H, channels=Cn, norm=norm)
    # the Python layer (value, gradient, level losses), at once under another stream: create returned with the handle usable on any stream
    got = run_on_stream(torch, B, form, [img, tgt], lambda: ms.value_and_grad(img.buf, tgt.buf, wc) + (ms.level_losses,), fetch, follows_at_once=True, returns_early=False)
    assert all(np.array_equal(a, b) for a, b in zip(got, base))
    pyr = run_on_stream(torch, B, form, [], lambda: ms.residual_pyramid(), fetch)
    pyr64 = ref.pyramid(img_np, tgt_np, W, H, wc_np)
    _check_values("70x45 l2 on a side stream, delay on %s" % form, (float(got[0]), got[2].astype(np.float64), got[1], pyr), pyr64, W, H, norm, wc_np, None)
    decoy = ref.evaluate(sc_.decoy_of(img_np), tgt_np, W, H, norm, wc_np)[0]
    assert abs(decoy - float(base[0])) > 1e-3          # (the decoy image is told apart)

    # the C ABI's eval: it returns while the delay is still running
    L = cabi.lib()
    out = torch.zeros(1 + ms.levels, device="cuda")
    grad = torch.zeros((W * H, Cn), device="cuda")

    def call():
        cabi.check(L.psdr_hip_msloss_eval(ms._handle.ptr, img.buf.data_ptr(), tgt.buf.data_ptr(), wc.data_ptr(), Cn, 1, None, out.data_ptr(), grad.data_ptr(),
                                          int(torch.cuda.current_stream().cuda_stream)))
        return out, grad
    o, g = run_on_stream(torch, B, form, [img, tgt], call, fetch, returns_early=True)
    assert np.array_equal(o[0], base[0]) and np.array_equal(o[1:], base[2]) and np.array_equal(g, base[1])

    # autograd under the stream (backward waits on the host for the engine's thread: no self-check)
    def autograd():
        leaf = img.buf.clone().requires_grad_()
        ms(leaf, tgt.buf, wc).backward()
        return leaf.grad
    assert np.array_equal(run_on_stream(torch, B, form, [img, tgt], autograd, lambda t: t.cpu().numpy(), returns_early=False), base[1])


def test_refusals(psdr):
    """the Python layer's ValueErrors and the C ABI's refusals that need a real handle; nothing here reaches a kernel"""
    import torch
    from psdr_jit_amd import cabi
    ms = psdr.MultiScaleLoss(37, 19)
    n = 37 * 19
    good = torch.zeros(n, 3)
    for img, tgt, w in ((torch.zeros(n, 4), good, None), (good, torch.zeros(n + 1, 3), None), (torch.zeros(n), good, None), (good, good, torch.zeros(n, 2)),
                        (good, good, torch.zeros(n + 1)), (torch.zeros(n, 3, dtype=torch.int32), good, None), (good, good, torch.zeros(n, dtype=torch.int64))):
        with pytest.raises(ValueError):
            ms(img, tgt, w)
    L = cabi.lib()
    hp = ms._handle.ptr
    x, y, w = (torch.zeros(n, 3, device="cuda") for _ in range(3))
    out, grad = torch.zeros(8, device="cuda"), torch.full((n, 3), 7.0, device="cuda")

    def refused(rc, name, word):
        msg = L.psdr_hip_last_error().decode()
        assert rc != 0 and msg.startswith(name + ":") and word in msg, (name, word, rc, msg)

    refused(L.psdr_hip_msloss_level(hp, 0, grad.data_ptr(), None), "psdr_hip_msloss_level", "has not been called")
    ev = L.psdr_hip_msloss_eval
    for wcn in (2, 4):
        refused(ev(hp, x.data_ptr(), y.data_ptr(), w.data_ptr(), wcn, 0, None, out.data_ptr(), grad.data_ptr(), None), "psdr_hip_msloss_eval", "weight_channels = %d, must be 0, 1 or C = 3" % wcn)
    refused(ev(hp, x.data_ptr(), y.data_ptr(), w.data_ptr(), 3, 2, None, out.data_ptr(), grad.data_ptr(), None), "psdr_hip_msloss_eval", "norm = 2")
    refused(ev(hp, x.data_ptr(), y.data_ptr(), None, 3, 0, None, out.data_ptr(), grad.data_ptr(), None), "psdr_hip_msloss_eval", "weight is NULL")
    refused(ev(hp, x.data_ptr(), y.data_ptr(), None, 0, 0, None, out.data_ptr(), x.data_ptr(), None), "psdr_hip_msloss_eval", "grad must be")
    lam = (C.c_float * 7)(1, 1, float("inf"), 1, 1, 1, 1)
    refused(ev(hp, x.data_ptr(), y.data_ptr(), None, 0, 0, lam, out.data_ptr(), grad.data_ptr(), None), "psdr_hip_msloss_eval", "level_weights[2]")
    refused(ev(hp, None, y.data_ptr(), None, 0, 0, None, out.data_ptr(), grad.data_ptr(), None), "psdr_hip_msloss_eval", "NULL")
    cabi.check(ev(hp, x.data_ptr(), y.data_ptr(), None, 0, 0, None, out.data_ptr(), None, None))
    for l in (-1, 7, 100):
        refused(L.psdr_hip_msloss_level(hp, l, grad.data_ptr(), None), "psdr_hip_msloss_level", "level = %d" % l)
    refused(L.psdr_hip_msloss_level(hp, 0, None, None), "psdr_hip_msloss_level", "out is NULL")
    h = C.c_void_p()
    refused(L.psdr_hip_msloss_create(37, 19, 8, 3, C.byref(h), None), "psdr_hip_msloss_create", "levels = 8")
    assert not h.value
    torch.cuda.synchronize()
    assert torch.equal(grad, torch.full((n, 3), 7.0, device="cuda")) and not out.any()
