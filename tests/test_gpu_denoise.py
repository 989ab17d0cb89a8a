"""GPU tests of the edge-avoiding a-trous denoiser (psdr_jit_amd/denoise.py, csrc/hip/denoise.hip) against the float64 restatement
tests/denoise_ref.py.

  1  exact: without guides and on images whose intermediate values all fit float32, the interior equals the restatement bit for bit
  2  apply and transpose against the restatement, element by element, within the bound derived below
  3  a constant image comes back, within the summation part of that bound
  4  <D x, y> = <x, D^T y>
  5  the non-finite-guide rule        6  the same call twice gives the same bits        7  autograd        8  end to end on a small box scene

Shapes are chosen at the tile's edges (a workgroup owns 32 x 8 pixels of one coset x = a, y = b mod s of the level's stride s): 1 x 1, 1 x 7 and 5 x 3 (smaller than
the taps' reach), 32 x 8 (one tile), 33 x 9 (one pixel more each way), 64 x 17 and 67 x 35 (several tiles, and at stride 2 a coset of 34 x 18: two tiles each way).
131 x 127 is added for test 1 only: the smallest frame with pixels whose 5 levels all stay inside it.

THE BOUND.  U = 2^-24 is float32's unit roundoff; everything is to first order in U.  One level of the kernel, for a pixel p, as the instructions are written:
  d2      G subtractions (each within U), G squares (U), G - 1 additions of non-negative terms (the first adds to 0): computed d2 = d2 (1 + t), |t| <= (G + 2) U
  exp     expf is documented to err by at most 1 ulp (HIP's device math functions), which is 2 U relative: E^ = exp(-d2 (1 + t)) (1 + 2 U).  The argument error changes
          the weight by d2 |t| exp(-d2) <= |t| sup d2 e^-d2 = |t| / e.  So |E^ - E| <= ((G + 2) / e + 2) U, and the product h(i) h(j) E^ (h h = k / 256 is exact) rounds
          once more: |w^ - w| <= h(i) h(j) c_G U,  c_G = (G + 2) / e + 3.  (A weight below 2^-126 may be flushed to 0: d2 > 87 there, where d2 e^-d2 < 1e-35 has left
          all of c_G unused.)  The centre tap is h(0)^2 exactly, and without guides d2 = 0, expf(-0) = 1 and every weight is exact: c_0 = 0.
  sums    S^ = the 25 products w^ x(q) (U each) added in 24 additions: within 25 U sum w^ |x(q)|.  N^ = the 25 weights added: N~ (1 + 24 U), N~ = sum w^.
  1 / N   one IEEE division (U) when the handle is made, one multiplication by it (U) per element.
So the computed A x (p) is within (25 + 24 + 1 + 1) U max|x| = 51 U max|x| of sum w^ x / N~, the level with the computed weights.  That one differs from the
exact level by the weights' errors, in the numerator and in the normaliser: 2 max|x| sum_q |w^ - w| / N <= 2 max|x| (55/64) c_G U / (9/64), with sum_{q != p} h h = 1 - 36/256
= 55/64 and N >= h(0)^2 = 9/64.  Together

    |computed A_l x (p) - A_l x (p)| <= K_G U max|x|,      K_G = 51 + (110 / 9) c_G        K_0 = 51,  K_1 = 101.2,  K_8 = 132.6

Every A_l is a convex combination, so it neither amplifies max|x| nor the error of the levels before it: |computed D x - D x| <= L K_G U max|x|, element by element.

The transpose level gathers T(p) = y(p) / N(p): T^ is within (24 + 1 + 1) U of y / N~, the sum adds 25 U: 51 U (A^T |y|)(q).  The weights' errors enter as
sum_p |w^(q, p) - w(q, p)| |y(p)| / N(p) <= (64/9) c_G U (Hb |y|)(q), Hb the unnormalised h(i) h(j) gather over the in-frame taps, and through 1 / N(p) as
(55/9) c_G U (A^T |y|)(q).  A^T is not a convex combination (its rows add up to as much as 64/9 beside an edge), so the bound is carried through the levels by the
restatement itself - all entries are non-negative, so |A^T e| <= A^T |e| - for l = L - 1 .. 0, from t = |y|, E = 0:
    E <- A_l^T E + U ((51 + (55/9) c_G) A_l^T t + (64/9) c_G Hb_l t),        t <- A_l^T t
and |computed D^T y - D^T y| <= E element by element (`adjoint_bound`).  The float64 restatement's own rounding, 2^-53 per operation, is 2^-29 of these and left out."""
import os

import numpy as np
import pytest

import denoise_ref as ref
import scenes
import test_denoise_cpu as cpu

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SHAPES = [(1, 1), (1, 7), (5, 3), (32, 8), (33, 9), (64, 17), (67, 35)]
FULL = [(33, 9), (67, 35)]                    # the shapes that run every C and G


def c_of(G):
    return (G + 2) / np.e + 3.0 if G else 0.0


def k_of(G):
    return 51.0 + (110.0 / 9.0) * c_of(G)


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists)")
    import __graft_entry__
    __graft_entry__.build()
    import psdr_jit_amd
    return torch, psdr_jit_amd


def _denoiser(env, g, W, H, L):
    torch, psdr = env
    return psdr.Denoiser(torch.from_numpy(g) if g is not None and g.shape[1] else None, W, H, levels=L)


def _run(env, den, x, adjoint=False):
    torch, _ = env
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    out = den.transpose(t) if adjoint else den(t)
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(t.shape)
    return out.cpu().numpy()


def adjoint_bound(y, g, W, H, L, G):
    """E of the module docstring: [W H, C]"""
    t = np.abs(np.asarray(y, np.float64)).reshape(H, W, -1)
    E = np.zeros_like(t)
    one = np.ones((H, W))
    c = c_of(G)
    for l in range(L - 1, -1, -1):
        w, N = ref.weights(g, W, H, l)
        w0, _ = ref.weights(None, W, H, l)
        At = ref._level(t, w, N, W, H, l, True)
        E = ref._level(E, w, N, W, H, l, True) + U * ((51.0 + 55.0 / 9.0 * c) * At + 64.0 / 9.0 * c * ref._level(t, w0, one, W, H, l, True))
        t = At
    return E.reshape(W * H, -1)


def _image(rng, n, C):
    """both signs, magnitudes over four decades"""
    return (rng.standard_normal((n, C)) * 10.0 ** rng.uniform(-2, 2, (n, 1))).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. exact
def _exact_image(rng, W, H, L):
    """[W H, 2], integer-valued and below 2^16.  A level multiplies by k / 256 and adds: it appends 8 binary places, so L levels of an image of b significant bits
    need b + 8 L <= 24 to stay exact in float32 (the restatement's float64 holds them all).  Channel 0 is random with b = 24 - 8 L bits: 16 bits for L = 1, multiples of
    256 for L = 2, {0, 2^15} for L = 3 (and for L > 3, where no random image stays exact: that channel is then only held to the bound).  Channel 1 is the quadratic
    x^2 + y^2 + x y + 3 x + 5 y, which stays exact at every depth: h has mean 0, second moment 1 and third moment 0, so a level of stride s maps it to itself + 2 s^2,
    integers again, through products and partial sums that are multiples of 1 / 256 below 2^16 - and a wrong stride, a wrong tap weight or a pixel taken from the wrong
    coset or halo slot changes that integer."""
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    bits = max(24 - 8 * L, 1)
    img = np.empty((H, W, 2), dtype=np.float32)
    img[..., 0] = rng.integers(0, 1 << bits, (H, W)) * float(1 << (16 - bits))
    img[..., 1] = xx * xx + yy * yy + xx * yy + 3 * xx + 5 * yy
    assert img.max() < 65536
    return img.reshape(W * H, 2)


@pytest.mark.parametrize("W,H,L", [(w, h, l) for (w, h) in SHAPES for l in (1, 3, 5)] + [(67, 35, 2), (67, 35, 4), (131, 127, 5)])
def test_exact_without_guides(env, W, H, L):
    """The pixels compared bit for bit are those whose taps - and the taps of the pixels they read, level by level - all lie inside the frame: at least
    m = 2 (2^L - 1) pixels from every border.  There N_l = 1 exactly at every level.  (A border pixel's 1 / N_l is rounded; those fall under the bound of test 2,
    which is asserted here as well.)  Frames without such pixels only run the bound."""
    rng = np.random.default_rng(W * 1000 + H * 10 + L)
    x = _exact_image(rng, W, H, L)
    got = _run(env, _denoiser(env, None, W, H, L), x)
    want = ref.apply(x, None, W, H, L)
    m = 2 * ((1 << L) - 1)
    inner = np.zeros((H, W), dtype=bool)
    if W > 2 * m and H > 2 * m:
        inner[m:H - m, m:W - m] = True
    inner = inner.reshape(-1)
    err = np.abs(got.astype(np.float64) - want)
    print("%d x %d, L = %d: %d interior pixels; largest error / bound elsewhere %.3g" % (W, H, L, inner.sum(), float(err.max()) / max(L * k_of(0) * U * float(np.abs(x).max()), 1e-300)))
    assert np.all(err <= L * k_of(0) * U * float(np.abs(x).max()))
    channels = [0, 1] if L <= 3 else [1]
    for c in channels:
        assert np.array_equal(got[inner, c].astype(np.float64), want[inner, c]), (c, np.nonzero(got[inner, c] != want[inner, c])[0][:8])
    if inner.any():
        yy, xx = np.divmod(np.nonzero(inner)[0], W)
        poly = xx * xx + yy * yy + xx * yy + 3 * xx + 5 * yy + 2 * sum(4 ** l for l in range(L))
        assert np.array_equal(got[inner, 1], poly.astype(np.float32))                  # the closed form: the restatement and the kernel are not wrong together


# ---------------------------------------------------------------------------------------------------------------------------
# 2. against the restatement
CASES = [(w, h, l, 3, 8) for (w, h) in SHAPES for l in (1, 3, 5)] + \
        [(w, h, l, c, g) for (w, h) in FULL for l in (1, 3, 5) for c in (1, 3, 4) for g in (0, 1, 8) if (c, g) != (3, 8)] + \
        [(67, 35, 2, 3, 8), (67, 35, 4, 2, 5)]


@pytest.mark.parametrize("W,H,L,C,G", CASES)
def test_apply_and_transpose_against_the_restatement(env, W, H, L, C, G):
    rng = np.random.default_rng(W * 10000 + H * 100 + L * 10 + C + G)
    g = cpu._guides(rng, W, H, G)
    x = _image(rng, W * H, C)
    den = _denoiser(env, g, W, H, L)
    got, want = _run(env, den, x), ref.apply(x, g, W, H, L)
    bound = L * k_of(G) * U * np.abs(x).max()
    err = np.abs(got.astype(np.float64) - want)
    got_t, want_t = _run(env, den, x, adjoint=True), ref.apply_adj(x, g, W, H, L)
    bound_t = adjoint_bound(x, g, W, H, L, G)
    err_t = np.abs(got_t.astype(np.float64) - want_t)
    print("%d x %d, L %d, C %d, G %d: apply error / bound %.3g (bound %.3g); transpose error / bound %.3g" %
          (W, H, L, C, G, err.max() / bound, bound, (err_t / np.maximum(bound_t, 1e-300)).max()))
    assert np.isfinite(got).all() and np.all(err <= bound), np.argwhere(err > bound)[:5]
    assert np.isfinite(got_t).all() and np.all(err_t <= bound_t), np.argwhere(err_t > bound_t)[:5]
    if G and W * H > 100:          # the guides matter: the same image filtered without them is not within the bound
        assert np.abs(ref.apply(x, None, W, H, L) - want).max() > 10 * bound


# ---------------------------------------------------------------------------------------------------------------------------
# 3. constants
@pytest.mark.parametrize("W,H", FULL)
def test_constants_come_back(env, W, H):
    """x = c: numerator and normaliser carry the SAME computed weights, so only the summation part of the bound is left: 51 U |c| per level"""
    rng = np.random.default_rng(W)
    for G in (0, 8):
        den = _denoiser(env, cpu._guides(rng, W, H, G), W, H, 5)
        c = np.float32([1.0, -3.7, 1.0e-3])
        got = _run(env, den, np.tile(c, (W * H, 1)))
        err = np.abs(got.astype(np.float64) - c.astype(np.float64))
        print("%d x %d, G %d: largest error / bound %.3g" % (W, H, G, (err / (5 * 51 * U * np.abs(c))).max()))
        assert np.all(err <= 5 * 51 * U * np.abs(c.astype(np.float64)))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the transpose identity
@pytest.mark.parametrize("W,H,L,C,G", [(33, 9, 5, 3, 8), (67, 35, 5, 4, 8), (67, 35, 3, 1, 1), (64, 17, 5, 3, 0), (5, 3, 3, 3, 8)])
def test_transpose_identity(env, W, H, L, C, G):
    """<D x, y> and <x, D^T y> in float64 from the device results agree within twice the relative bound of test 2, L K_G U, times sum |x| |y|"""
    rng = np.random.default_rng(W + H + L + C + G)
    g = cpu._guides(rng, W, H, G)
    x, y = rng.standard_normal((W * H, C)).astype(np.float32), rng.standard_normal((W * H, C)).astype(np.float32)
    den = _denoiser(env, g, W, H, L)
    lhs = float((_run(env, den, x).astype(np.float64) * y).sum())
    rhs = float((x.astype(np.float64) * _run(env, den, y, adjoint=True)).sum())
    tol = 2 * L * k_of(G) * U * float((np.abs(x).astype(np.float64) * np.abs(y)).sum())
    # (the bound that follows element by element from test 2's, for comparison: sum |y| (apply's bound) + sum |x| (the transpose's))
    rigorous = float(L * k_of(G) * U * np.abs(x).max() * np.abs(y).sum() + (np.abs(x) * adjoint_bound(y, g, W, H, L, G)).sum())
    print("%d x %d, L %d, C %d, G %d: %.9g against %.9g, difference %.3g, bound %.3g (element-wise bounds added up: %.3g)" % (W, H, L, C, G, lhs, rhs, abs(lhs - rhs), tol, rigorous))
    assert abs(lhs - rhs) <= tol


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the non-finite-guide rule
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("where", ["interior", "corner"])
def test_non_finite_guide(env, bad, where):
    """a non-finite guide value at q zeroes exactly the taps that touch q and leaves q's own centre tap: the result is finite and within the bound of the restatement
    (which states the rule); q's value reaches no other pixel (another value at q changes the output at q alone, bit for bit) and q sees no other pixel"""
    W, H, L, G, C = 33, 9, 3, 3, 3
    rng = np.random.default_rng(17)
    g = cpu._guides(rng, W, H, G) * np.float32(0.1)
    qx, qy = (20, 4) if where == "interior" else (0, 0)
    q = qy * W + qx
    g[q, 1] = bad
    den = _denoiser(env, g, W, H, L)
    x = _image(rng, W * H, C)
    got, want = _run(env, den, x), ref.apply(x, g, W, H, L)
    bound = L * k_of(G) * U * np.abs(x).max()
    assert np.isfinite(got).all() and np.all(np.abs(got - want) <= bound)
    x2 = x.copy()
    x2[q] = [1.0e3, -2.0e3, 5.0e2]
    got2 = _run(env, den, x2)
    others = np.arange(W * H) != q
    assert np.array_equal(got[others], got2[others]) and not np.array_equal(got[q], got2[q])
    assert np.all(np.abs(got2[q].astype(np.float64) - x2[q]) <= L * 51 * U * np.abs(x2[q]))          # every level hands q back: x h(0)^2 / h(0)^2
    got_t, want_t = _run(env, den, x, adjoint=True), ref.apply_adj(x, g, W, H, L)
    assert np.isfinite(got_t).all() and np.all(np.abs(got_t - want_t) <= adjoint_bound(x, g, W, H, L, G))


# ---------------------------------------------------------------------------------------------------------------------------
# 6. determinism, 7. autograd
def test_same_bits_twice_and_autograd(env):
    torch, psdr = env
    W, H, L, G, C = 67, 35, 5, 8, 3
    rng = np.random.default_rng(23)
    den = _denoiser(env, cpu._guides(rng, W, H, G), W, H, L)
    x = torch.from_numpy(_image(rng, W * H, C)).cuda()
    gy = torch.from_numpy(_image(rng, W * H, C)).cuda()
    a, b = den(x), den(x)
    ta, tb = den.transpose(gy), den.transpose(gy)
    assert torch.equal(a, b) and torch.equal(ta, tb)
    again = psdr.Denoiser(torch.from_numpy(cpu._guides(np.random.default_rng(23), W, H, G)), W, H, levels=L)          # another handle from the same guides
    assert torch.equal(again(x), a) and torch.equal(again.transpose(gy), ta)
    img = x.clone().requires_grad_()
    out = den(img)
    assert out.requires_grad and torch.equal(out.detach(), a)
    out.backward(gy)
    assert torch.equal(img.grad, ta)
    # a [n, C] view that is not contiguous, and a float64 image: made contiguous float32 on the way in, the gradient goes back in the input's type
    wide = torch.zeros((W * H, 2 * C), device="cuda", dtype=torch.float64)
    wide[:, ::2] = x.double()
    leaf = wide.requires_grad_()
    den(leaf[:, ::2]).backward(gy)
    assert leaf.grad.dtype == torch.float64 and torch.equal(leaf.grad[:, ::2], ta.double()) and float(leaf.grad[:, 1::2].abs().max()) == 0.0
    with pytest.raises(ValueError, match="expected"):
        den(torch.zeros((W * H, 5), device="cuda"))
    with pytest.raises(ValueError, match="expected"):
        den(torch.zeros((W * H + 1, 3), device="cuda"))


# ---------------------------------------------------------------------------------------------------------------------------
# 8. end to end
W8 = H8 = 32
LOW_SPP, TRUTH_SPP = 2, 1024


@pytest.fixture(scope="module")
def box(env):
    import product
    return product.build_scene(scenes.cbox_scene(W8, H8, spp=LOW_SPP, param=None))


def _set_spp(sc, spp):
    sc.opts.spp = spp
    sc.configure(sc.__dict__.get("_psdr_active", []))


def test_first_hit_guides_are_the_scaled_field_renders(env, box):
    torch, psdr = env
    sc, n = box, W8 * H8
    fields = ("silhouette", "shNormal", "position")
    g = psdr.first_hit_guides(sc, seed=3)
    renders = {f: psdr.FieldExtractionIntegrator(f).renderC(sc, 0, seed=3) for f in fields}
    hit = renders["silhouette"][:, 0] > 0
    pos = renders["position"][hit]
    extent = float((pos.max(dim=0).values - pos.min(dim=0).values).max())
    sig = {"silhouette": 0.1, "shNormal": 0.25, "position": 0.05 * extent}
    want = torch.cat([renders[f][:, :psdr.denoise.FIELD_CHANNELS[f]] / (sig[f] * 2.0 ** 0.5) for f in fields], dim=1)
    assert tuple(g.shape) == (n, 7) and g.dtype == torch.float32 and not g.requires_grad and n // 4 < int(hit.sum()) < n and extent > 100.0          # (the box fills a good third of the frame)
    # one division by a float32 scale that is itself a rounded product: 4 U relative covers both sides
    assert float(((g - want).abs() - 4 * U * want.abs()).max()) <= 0.0
    g2 = psdr.first_hit_guides(sc, seed=3, fields=("depth", "bsdf", "uv"), sigma={"bsdf": 0.5, "depth": 7.0})
    depth = psdr.FieldExtractionIntegrator("depth").renderC(sc, 0, seed=3)[:, :1]
    bsdf = psdr.FieldExtractionIntegrator("bsdf").renderC(sc, 0, seed=3)
    assert tuple(g2.shape) == (n, 6)
    assert float(((g2[:, :1] - depth / (7.0 * 2.0 ** 0.5)).abs() - 4 * U * g2[:, :1].abs()).max()) <= 0.0
    assert float(((g2[:, 1:4] - bsdf / (0.5 * 2.0 ** 0.5)).abs() - 4 * U * g2[:, 1:4].abs()).max()) <= 0.0


def test_denoised_low_spp_render_is_closer_to_the_truth(env, box):
    """renderC at 2 spp (seed 5) against 1024 spp (seed 11), guides from seed 3, L = 5.  On the CPU - the oracle's renders of the same scene with the same seeds, its
    field renders scaled by first_hit_guides' rule, put through tests/denoise_ref.py - MSE(noisy) = 0.13396, MSE(denoised) = 0.05706: a ratio of 0.426, below one half.
    (Position's default sigma is tight for a frame this coarse - neighbouring pixels are 17 scene units apart, sigma is 28 - so levels 3 and 4 add nothing here: L = 3
    gives the same ratio.)  The assertion here is the plain inequality."""
    torch, psdr = env
    sc = box
    integ = psdr.PathTracer(2)
    den = psdr.Denoiser(psdr.first_hit_guides(sc, seed=3), W8, H8, levels=5)
    noisy = integ.renderC(sc, 0, seed=5)
    try:
        _set_spp(sc, TRUTH_SPP)
        truth = integ.renderC(sc, 0, seed=11)
    finally:
        _set_spp(sc, LOW_SPP)
    out = den(noisy)
    mse_noisy, mse_den = float(((noisy - truth) ** 2).mean()), float(((out - truth) ** 2).mean())
    print("MSE against %d spp: %d spp %.5g, denoised %.5g, ratio %.3f" % (TRUTH_SPP, LOW_SPP, mse_noisy, mse_den, mse_den / mse_noisy))
    assert mse_noisy > 0 and mse_den < mse_noisy


def test_backward_through_the_denoiser_is_the_hand_written_adjoint(env):
    """loss(den(renderD(...))).backward() against den.transpose(dloss / dout) fed into img.backward(...) by hand.

    The gradient that reaches the render is the same tensor bit for bit: that is all of the denoiser's part, and it is asserted so.  The leaf gradient behind it is
    NOT bit for bit, although both ways hand the same bits to the same reverse pass: renderD's reverse pass adds its N samples' shares with float atomics in an
    order of its own in every run (tests/test_gpu_adaptive.py::test_differentiable_recipe states and bounds the same thing).  Measured on an MI355X: 4.98430204
    against 4.98430157.  So the two leaf gradients are held to that test's order-free bound instead: each is within (N - 1) U sum |shares| of the exact sum, the
    two within 2 (N + 1) U A of each other, with A = sum_p,c |dloss/dimg[p, c] d img[p, c] / dP| (from forward_grad) standing for the sum of the absolute
    shares and N = W H spp interior samples + W H (sppe + sppse) edge samples."""
    torch, psdr = env
    from test_gpu_adaptive import _moving_box_scene
    width, height, spp = 32, 32, 2
    P = psdr.FloatD(0.).requires_grad_()
    sc = _moving_box_scene(psdr, P, width, height, spp)
    integ = psdr.PathTracer(2)
    den = psdr.Denoiser(psdr.first_hit_guides(sc, seed=3), width, height, levels=5)
    w = torch.linspace(0.5, 1.5, width * height * 3, device="cuda").reshape(-1, 3)
    seen = []

    img = integ.renderD(sc, 0, seed=7)
    img.register_hook(lambda grad: seen.append(grad.clone()))
    d_img = psdr.forward_grad(img, P).detach()                 # (before any backward() frees the graph from P to the mesh transform)
    (den(img) * w).sum().backward(retain_graph=True)          # (that graph is shared with the second render below)
    got = P.grad.clone()
    P.grad = None

    img2 = integ.renderD(sc, 0, seed=7)
    assert torch.equal(img2.detach(), img.detach())
    by_hand = den.transpose(w)
    img2.backward(by_hand)
    want = P.grad.clone()
    assert len(seen) == 1 and torch.equal(seen[0], by_hand)
    A = float((by_hand.double() * d_img.double()).abs().sum())
    N = width * height * spp + width * height * 2 * spp
    tol = 2 * (N + 1) * U * A
    print("dP through the denoiser %.9g, by hand %.9g, difference %.3g, bound %.3g; A = %.4g" % (float(got), float(want), abs(float(got) - float(want)), tol, A))
    assert A > 0 and float(want) != 0.0 and abs(float(got) - float(want)) <= tol
    # the forward derivative of the denoised image is the denoised forward derivative (D is linear): <w, D d_img> is the gradient forward mode sees
    fwd = float((den(d_img).double() * w.double()).sum())
    assert abs(fwd - float(want)) < 1e-2 * A
