"""GPU tests of the SSIM loss (psdr_jit_amd/ssim.py, csrc/hip/ssim.hip) against the float64 checker tests/ssim_ref.py: the map S, the mean, the loss and every gradient
entry within the checker's derived bound (ssim_ref.bounds: u = 2^-24, gamma_{2K} per window sum, a value-with-bound arithmetic through the definition; nothing is
tuned and nothing is left out), on uniform and on nearly flat inputs, without a mask, with a mask of zeros and with a fractional one, both paddings; identical images,
an all-zero mask, repeatability, handle state, autograd (down to the parameter of a rendered scene), streams and every refusal that needs a real handle.

Shapes (W x H; the kernels' tile is 32 x 16): 1 x 1 all halo; 2 x 7 and 7 x 2 smaller than R each way; 11 x 11 the first frame "valid" accepts at K = 11, exactly one
pixel counts; 32 x 16 exactly one tile; 33 x 17 one tile plus one pixel in each direction; 37 x 19; 70 x 45 (3 x 3 partial tiles); 96 x 32 three tiles wide and two
high: the middle tiles' halo crosses a tile border on either side.  C = 3 everywhere, C = 1 and 4 on 33 x 17 and 70 x 45; K in {3, 7, 11}; sigma 1.5 and 0.5.

The worst error / bound seen on an MI355X (printed by test_values, recorded in DESIGN.md section 7i): S 0.26, mean 0.03, loss 0.03, gradient 0.41."""
import ctypes as C

import numpy as np
import pytest

import ssim_ref as ref
from stream_cases import Slot, run_on_stream, run_plain

pytestmark = pytest.mark.gpu

TILE_W, TILE_H = 32, 16
SHAPES = [(1, 1), (2, 7), (7, 2), (11, 11), (TILE_W, TILE_H), (TILE_W + 1, TILE_H + 1), (37, 19), (70, 45), (3 * TILE_W, 2 * TILE_H)]
CASES = [(W, H, 3) for W, H in SHAPES] + [(33, 17, 1), (33, 17, 4), (70, 45, 1), (70, 45, 4)]
WINDOWS = (3, 7, 11)
SIGMAS = (1.5, 0.5)
WORST = {}


@pytest.fixture(scope="module")
def psdr():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists)")
    import __graft_entry__
    __graft_entry__.build()
    import psdr_jit_amd
    return psdr_jit_amd


def _run(ss, img, tgt, mask):
    """(loss, mean, gradient, map) of the device, as numpy"""
    import torch
    t = lambda a: None if a is None else torch.from_numpy(a).cuda()
    loss, grad = ss.value_and_grad(t(img), t(tgt), t(mask))
    assert loss.is_cuda and loss.dim() == 0 and loss.dtype == torch.float32 and tuple(grad.shape) == img.shape and grad.dtype == torch.float32
    assert ss.ssim.dim() == 0 and ss.ssim.is_cuda and not ss.ssim.requires_grad
    smap = ss.ssim_map()
    assert tuple(smap.shape) == img.shape
    return float(loss.cpu()), float(ss.ssim.cpu()), grad.cpu().numpy(), smap.cpu().numpy()


def _check(label, got, b):
    """every quantity of the device within the checker's bound, every entry; -> the worst error / bound per quantity"""
    loss, mean, grad, smap = got
    worst = {}
    for name, have, vb in (("S", smap, b["S"]), ("grad", grad, b["grad"]), ("mean", np.float64(mean), b["mean"]), ("loss", np.float64(loss), b["loss"])):
        have = np.asarray(have, np.float64)
        err = np.abs(have - vb.v)
        worst[name] = float((err / np.maximum(vb.e, 1e-300)).max())
        assert np.isfinite(have).all() and np.all(err <= vb.e), (label, name, worst[name], float(err.max()))
    return worst


@pytest.mark.parametrize("K", WINDOWS)
@pytest.mark.parametrize("W,H,Cn", CASES)
def test_values(psdr, W, H, Cn, K):
    binary, frac = ref.masks(W, H)
    inputs = (("uniform", ref.uniform_inputs(W, H, Cn)), ("flat", ref.flat_inputs(W, H, Cn)))
    worst = {}
    for sigma in SIGMAS:
        for padding in ("same", "valid"):
            if padding == "valid" and (W < K or H < K):
                with pytest.raises(ValueError):
                    psdr.SSIMLoss(W, H, channels=Cn, window=K, sigma=sigma, padding=padding)
                continue
            ss = psdr.SSIMLoss(W, H, channels=Cn, window=K, sigma=sigma, padding=padding)
            assert ss.taps.tobytes() == ref.taps(K, sigma).tobytes()
            for kind, (img, tgt) in inputs:
                for mname, mask in (("none", None), ("zeros", binary), ("fractional", frac)):
                    label = "%dx%d C=%d K=%d sigma=%g %s %s mask %s" % (W, H, Cn, K, sigma, padding, kind, mname)
                    b = ref.bounds(img, tgt, W, H, K, sigma, mask=mask, padding=padding)
                    got = _run(ss, img, tgt, mask.reshape(-1) if mname == "fractional" else mask)
                    for name, r in _check(label, got, b).items():
                        worst[name] = max(worst.get(name, 0.0), r)
                    if mname == "zeros":
                        # no unmasked pixel within R: every term of the gradient is 0 (the bound keeps only its underflow terms), and so is the gradient - exactly
                        m_eff = ref.effective_mask(W, H, K, mask, padding)
                        dead = (ref.window_sum((m_eff > 0).astype(np.float64), np.ones(K)) == 0).reshape(-1)
                        assert np.all(b["grad"].e[dead] < 1e-40) and not got[2][dead].any()
                        if W >= 2 * TILE_W and H >= 2 * TILE_H:
                            assert dead.any(), label
                    if padding == "valid" and (W, H, K) == (11, 11, 11) and mask is None:
                        # exactly one pixel counts: the mean is that pixel's S over the channels
                        centre = got[3].reshape(H, W, Cn)[5, 5].astype(np.float64)
                        assert abs(got[1] - centre.mean()) <= 4 * ref.U * np.abs(centre).mean()
    print("%dx%d C=%d K=%d: worst error / bound %s" % (W, H, Cn, K, "  ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    for name, r in worst.items():
        WORST[name] = max(WORST.get(name, 0.0), r)
    print("so far, all cases: %s" % "  ".join("%s %.3f" % kv for kv in sorted(WORST.items())))


@pytest.mark.parametrize("K,sigma", [(11, 1.5), (3, 1.5), (7, 0.5)])
def test_identical_images_and_empty_mask(psdr, K, sigma):
    import torch
    for W, H, Cn, gen in ((37, 19, 3, ref.uniform_inputs), (70, 45, 4, ref.flat_inputs), (2, 7, 1, ref.uniform_inputs)):
        img, tgt = gen(W, H, Cn)
        ss = psdr.SSIMLoss(W, H, channels=Cn, window=K, sigma=sigma)
        loss, mean, grad, smap = _run(ss, img, img.copy(), None)
        assert np.all(smap == 1.0) and abs(loss) <= 2.0 ** -23 and abs(mean - 1.0) <= 2.0 ** -23
        b = ref.bounds(img, img, W, H, K, sigma)
        assert np.abs(b["grad"].v).max() <= 1e-12 and np.all(np.abs(grad.astype(np.float64) - b["grad"].v) <= b["grad"].e)
        # an all-zero mask: N == 0, out == (0, 0) and the gradient is 0, exactly; the map is the unmasked one
        sentinel = torch.full((W * H, Cn), 7.0, device="cuda")
        out = torch.full((2,), 7.0, device="cuda")
        x, y, zero = torch.from_numpy(img).cuda(), torch.from_numpy(tgt).cuda(), torch.zeros(W * H, device="cuda")
        from psdr_jit_amd import cabi
        cabi.check(cabi.lib().psdr_hip_ssim_eval(ss._handle.ptr, x.data_ptr(), y.data_ptr(), zero.data_ptr(), out.data_ptr(), sentinel.data_ptr(), None))
        torch.cuda.synchronize()
        assert out.tolist() == [0.0, 0.0] and not sentinel.any()
        loss, mean, grad, smap0 = _run(ss, img, tgt, np.zeros((W * H, 1), np.float32))
        assert loss == 0.0 and mean == 0.0 and not grad.any()
        assert np.array_equal(smap0, _run(ss, img, tgt, None)[3])


def test_same_bits_every_call_and_no_state_left(psdr):
    import torch
    W, H, Cn = 70, 45, 3
    binary, frac = (torch.from_numpy(m).cuda() for m in ref.masks(W, H))
    a_img, a_tgt = (torch.from_numpy(x).cuda() for x in ref.uniform_inputs(W, H, Cn, seed=2))
    b_img, b_tgt = (torch.from_numpy(x).cuda() for x in ref.flat_inputs(W, H, Cn, seed=3))
    for padding in ("same", "valid"):
        ss = psdr.SSIMLoss(W, H, channels=Cn, padding=padding)
        la, ga = ss.value_and_grad(a_img, a_tgt, frac)
        ma, sa = ss.ssim, ss.ssim_map()
        lb, gb = ss.value_and_grad(b_img, b_tgt)                      # another pair, no mask, on the same handle
        assert not torch.equal(la, lb) and not torch.equal(ga, gb) and not torch.equal(sa, ss.ssim_map())
        la2, ga2 = ss.value_and_grad(a_img, a_tgt, frac)
        assert torch.equal(la, la2) and torch.equal(ga, ga2) and torch.equal(ma, ss.ssim) and torch.equal(sa, ss.ssim_map())
        fresh = psdr.SSIMLoss(W, H, channels=Cn, padding=padding)
        lf, gf = fresh.value_and_grad(a_img, a_tgt, frac)
        assert torch.equal(la, lf) and torch.equal(ga, gf) and torch.equal(sa, fresh.ssim_map())
        # grad = NULL: the same out bits, and the map of that call
        out, none = ss._eval(b_img, b_tgt, None, False)
        assert none is None and torch.equal(out[0], lb)
        out, none = ss._eval(a_img, a_tgt, frac, False)
        assert torch.equal(out[0], la) and torch.equal(out[1], ma) and torch.equal(sa, ss.ssim_map())


def test_autograd(psdr):
    import torch
    W, H, Cn = 37, 19, 3
    img, tgt = (torch.from_numpy(x).cuda() for x in ref.uniform_inputs(W, H, Cn, seed=4))
    mask = torch.from_numpy(ref.masks(W, H)[1]).cuda()
    ss = psdr.SSIMLoss(W, H, channels=Cn)
    loss, g = ss.value_and_grad(img, tgt, mask)
    assert not loss.requires_grad and not g.requires_grad
    x, t, m = img.clone().requires_grad_(), tgt.clone().requires_grad_(), mask.clone().requires_grad_()
    out = ss(x, t, m)
    assert out.dim() == 0 and out.requires_grad and torch.equal(out.detach(), loss) and not ss.ssim.requires_grad
    out.backward()
    assert torch.equal(x.grad, g) and t.grad is None and m.grad is None and float(g.abs().max()) > 0
    x2 = img.clone().requires_grad_()
    (3.0 * ss(x2, tgt, mask)).backward()
    assert torch.equal(x2.grad, 3.0 * g)
    # a CPU float64 leaf gets a CPU float64 gradient
    x64 = img.cpu().double().requires_grad_()
    ss(x64, tgt, mask).backward()
    assert x64.grad.device.type == "cpu" and x64.grad.dtype == torch.float64 and torch.equal(x64.grad, g.cpu().double())


def test_gradient_reaches_the_scene_parameter(psdr):
    """the README box at 32 x 32 and 2 spp: P.grad through ss equals P.grad of <g, renderD> with g the fused image gradient, bit for bit - the reverse sweep is
    deterministic and backward hands it g times exactly 1"""
    import torch
    import test_gpu_api as api
    grads = []
    for use_ss in (True, False):
        P = psdr.FloatD(0.).requires_grad_()
        sc = api._readme_scene(psdr, P, res=32, spp=2)
        integ = psdr.PathTracer(2)
        ss = psdr.SSIMLoss(32, 32)
        if not grads:
            target = 0.5 * integ.renderC(sc, 0, seed=3)
        img = integ.renderD(sc, 0, seed=11)
        if use_ss:
            ss(img, target).backward()
        else:
            _loss, g = ss.value_and_grad(img.detach(), target)
            (g.detach() * img).sum().backward()
        grads.append(P.grad.detach().cpu().clone())
    print("P.grad", float(grads[0]), float(grads[1]))
    assert torch.equal(grads[0], grads[1]) and float(grads[0]) != 0.0 and np.isfinite(float(grads[0]))


@pytest.mark.parametrize("form", ("S", "default"))
def test_made_on_one_stream_evaluated_on_another(psdr, form):
    import torch
    from psdr_jit_amd import cabi
    import stream_cases as sc_
    W, H, Cn = 70, 45, 3
    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    img_np, other = ref.uniform_inputs(W, H, Cn, seed=5)
    tgt_np = (0.75 * img_np + 0.25 * other).astype(np.float32)          # close to img: the rolled decoy of either is far from it
    mask_np = ref.masks(W, H, seed=5)[1]
    img, tgt = Slot(torch, img_np), Slot(torch, tgt_np)
    mask = torch.from_numpy(mask_np).cuda()
    plain = psdr.SSIMLoss(W, H, channels=Cn)
    fetch = lambda o: [t.cpu().numpy() for t in o]
    base = run_plain(torch, [img, tgt], lambda: plain.value_and_grad(img.buf, tgt.buf, mask) + (plain.ssim, plain.ssim_map()), fetch)
    for s in (img, tgt):
        s.reset()
    torch.cuda.synchronize()
    with torch.cuda.stream(A):
        sc_.delay(torch)
        ss = psdr.SSIMLoss(W, H, channels=Cn)
    # the Python layer (value, gradient, mean), at once under another stream: create returned with the handle usable on any stream
    got = run_on_stream(torch, B, form, [img, tgt], lambda: ss.value_and_grad(img.buf, tgt.buf, mask) + (ss.ssim,), fetch, follows_at_once=True, returns_early=False)
    assert all(np.array_equal(a, b) for a, b in zip(got, base[:3]))
    smap = run_on_stream(torch, B, form, [], lambda: (ss.ssim_map(),), fetch)[0]
    assert np.array_equal(smap, base[3])
    _check("70x45 on a side stream, delay on %s" % form, (float(got[0]), float(got[2]), got[1], smap), ref.bounds(img_np, tgt_np, W, H, mask=mask_np))
    decoy = ref.evaluate(sc_.decoy_of(img_np), tgt_np, W, H, mask=mask_np)[0]
    assert abs(decoy - float(base[0])) > 1e-3          # (the decoy image is told apart)

    # the C ABI's eval: it returns while the delay is still running
    L = cabi.lib()
    out = torch.zeros(2, device="cuda")
    grad = torch.zeros((W * H, Cn), device="cuda")

    def call():
        cabi.check(L.psdr_hip_ssim_eval(ss._handle.ptr, img.buf.data_ptr(), tgt.buf.data_ptr(), mask.data_ptr(), out.data_ptr(), grad.data_ptr(),
                                        int(torch.cuda.current_stream().cuda_stream)))
        return out, grad
    o, g = run_on_stream(torch, B, form, [img, tgt], call, fetch, returns_early=True)
    assert np.array_equal(o[0], base[0]) and np.array_equal(o[1], base[2]) and np.array_equal(g, base[1])

    # the map's copy returns early too
    def copy_map():
        s = torch.empty((W * H, Cn), device="cuda")
        cabi.check(L.psdr_hip_ssim_map(ss._handle.ptr, s.data_ptr(), int(torch.cuda.current_stream().cuda_stream)))
        return (s,)
    assert np.array_equal(run_on_stream(torch, B, form, [], copy_map, fetch, returns_early=True)[0], base[3])

    # autograd under the stream (backward waits on the host for the engine's thread: no self-check)
    def autograd():
        leaf = img.buf.clone().requires_grad_()
        ss(leaf, tgt.buf, mask).backward()
        return leaf.grad
    assert np.array_equal(run_on_stream(torch, B, form, [img, tgt], autograd, lambda t: t.cpu().numpy(), returns_early=False), base[1])


def test_refusals(psdr):
    """the Python layer's ValueErrors and the C ABI's refusals that need a real handle; nothing here reaches a kernel"""
    import torch
    from psdr_jit_amd import cabi
    ss = psdr.SSIMLoss(37, 19)
    n = 37 * 19
    good = torch.zeros(n, 3)
    for img, tgt, m in ((torch.zeros(n, 4), good, None), (good, torch.zeros(n + 1, 3), None), (torch.zeros(n), good, None), (good, good, torch.zeros(n, 3)),
                        (good, good, torch.zeros(n, 2)), (good, good, torch.zeros(n + 1)), (torch.zeros(n, 3, dtype=torch.int32), good, None),
                        (good, good, torch.zeros(n, dtype=torch.int64)), (good.numpy(), good, None), (good, good, np.zeros(n, np.float32))):
        with pytest.raises(ValueError):
            ss(img, tgt, m)
        with pytest.raises(ValueError):
            ss.value_and_grad(img, tgt, m)
    for kw in (dict(padding="reflect"), dict(channels=5), dict(window=4), dict(window=13), dict(sigma=0.0), dict(k1=0.0), dict(data_range=float("inf"))):
        with pytest.raises(ValueError):
            psdr.SSIMLoss(37, 19, **kw)
    for W, H, K in ((10, 11, 11), (37, 6, 7), (0, 19, 11), (4097, 4096, 11)):
        with pytest.raises(ValueError):
            psdr.SSIMLoss(W, H, window=K, padding="valid")
    L = cabi.lib()
    hp = ss._handle.ptr
    x, y = (torch.zeros(n, 3, device="cuda") for _ in range(2))
    out, grad = torch.full((2,), 7.0, device="cuda"), torch.full((n, 3), 7.0, device="cuda")

    def refused(rc, name, word):
        msg = L.psdr_hip_last_error().decode()
        assert rc != 0 and msg.startswith(name + ":") and word in msg, (name, word, rc, msg)

    refused(L.psdr_hip_ssim_map(hp, grad.data_ptr(), None), "psdr_hip_ssim_map", "has not been called")
    ev = L.psdr_hip_ssim_eval
    refused(ev(hp, None, y.data_ptr(), None, out.data_ptr(), grad.data_ptr(), None), "psdr_hip_ssim_eval", "NULL")
    refused(ev(hp, x.data_ptr(), None, None, out.data_ptr(), grad.data_ptr(), None), "psdr_hip_ssim_eval", "NULL")
    refused(ev(hp, x.data_ptr(), y.data_ptr(), None, None, grad.data_ptr(), None), "psdr_hip_ssim_eval", "NULL")
    refused(ev(hp, x.data_ptr(), y.data_ptr(), None, out.data_ptr(), x.data_ptr(), None), "psdr_hip_ssim_eval", "grad must be")
    refused(ev(hp, x.data_ptr(), y.data_ptr(), None, out.data_ptr(), y.data_ptr(), None), "psdr_hip_ssim_eval", "grad must be")
    refused(ev(None, x.data_ptr(), y.data_ptr(), None, out.data_ptr(), grad.data_ptr(), None), "psdr_hip_ssim_eval", "handle is NULL")
    refused(L.psdr_hip_ssim_map(hp, grad.data_ptr(), None), "psdr_hip_ssim_map", "has not been called")          # (a refused eval does not count)
    refused(L.psdr_hip_ssim_map(hp, None, None), "psdr_hip_ssim_map", "out is NULL")
    h = C.c_void_p()
    taps = (C.c_float * 11)(*[float(v) for v in ref.taps(11, 1.5)])
    c1, c2 = (float(c) for c in ref.constants())
    create = L.psdr_hip_ssim_create
    refused(create(37, 19, 3, 10, taps, c1, c2, 0, C.byref(h), None), "psdr_hip_ssim_create", "window = 10")
    refused(create(37, 19, 5, 11, taps, c1, c2, 0, C.byref(h), None), "psdr_hip_ssim_create", "C = 5")
    refused(create(37, 19, 3, 11, taps, 0.0, c2, 0, C.byref(h), None), "psdr_hip_ssim_create", "c1 =")
    refused(create(37, 19, 3, 11, taps, c1, c2, 2, C.byref(h), None), "psdr_hip_ssim_create", "padding = 2")
    refused(create(37, 10, 3, 11, taps, c1, c2, 1, C.byref(h), None), "psdr_hip_ssim_create", "valid padding")
    refused(create(37, 19, 3, 9, taps, c1, c2, 0, C.byref(h), None), "psdr_hip_ssim_create", "sum to")
    assert not h.value
    torch.cuda.synchronize()
    assert torch.equal(grad, torch.full((n, 3), 7.0, device="cuda")) and torch.equal(out, torch.full((2,), 7.0, device="cuda"))
