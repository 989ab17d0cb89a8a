"""GPU tests of the variance-guided a-trous denoiser (psdr_jit_amd/vdenoise.py, csrc/hip/vdenoise.hip) against the float64 restatement
tests/vdenoise_ref.py.

  1  apply (image and variance) against the restatement, within a tolerance taken from the restatement alone
  2  frozen and frozen_transpose against the restatement fed the DEVICE'S OWN recorded planes, within the bound derived below
  3  <D_x u, y> = <u, D_x^T y>          4  sigma_l = inf gives psdr.Denoiser's bits          5  bit equalities: frozen(img), twice, autograd, a replaced record
  6  the non-finite rule                7  the step frames of the issue                      8  end to end on a small box scene

Shapes as in tests/test_gpu_denoise.py, at the tile's edges (a workgroup owns 32 x 8 pixels of one coset of the level's stride).

TEST 1'S TOLERANCE.  The map is not linear and exp(-z) is steep, so no closed bound is written down.  The restatement is run eight more times in float64 on inputs whose
every element (image, variance, guides) is multiplied by 1 + 2^-23 or 1 - 2^-23, signs random, seeds fixed: spread(p) is the largest distance of those eight from the
plain run at p, that is what one unit of float32 input rounding does to the answer.  The device must satisfy |got - want|(p) <= 16 max(spread(p), 4 x 2^-24 max|x|)
(for the variance: max v in the floor).  16 and 4 x 2^-24 are the project's margin and floor of the lane and adjoint measures; they were not tuned on this kernel.

TEST 2'S BOUND.  U = 2^-24, everything to first order in U, as in tests/test_gpu_denoise.py, whose K_G = 51 + (110 / 9) c_G is extended by what z adds.  The frozen
modes read lum, vt and 1 / N from the record, and the restatement is fed the same planes, so forming lum (C multiplications and additions) is not part of the difference.
  d2      as there: d2 (1 + t1), |t1| <= (G + 2) U, and exactly 0 without guides
  z       dl = lum(p) - lum(q) (U), its square (U, on a value carrying 2 U): 3 U; times k (U): 4 U; vt(p) + vt(q) (U), + eps (U), all terms non-negative: 2 U; the
          division (U): z (1 + t2), |t2| <= 7 U
  d2 + z  both non-negative, one addition (U): the exponent's argument is (d2 + z) (1 + t), |t| <= tau_G U, tau_G = max(G + 2, 7) + 1, and tau_0 = 7 (0 + z is exact)
  exp     1 ulp = 2 U, the argument's error costs at most |t| sup a e^-a = |t| / e, the product with h(i) h(j) rounds once more:
          |w^ - w| <= h(i) h(j) c'_G U,  c'_G = tau_G / e + 3          c'_0 = 5.58, c'_1 = 5.94, c'_8 = 7.05
  sums    25 products (U each) in 24 additions, one multiplication by the recorded 1 / N: 26 U sum w^ |u(q)| / N.  1 / N is the SAME number on both sides, so the
          normaliser carries no error of its own; the weights' errors enter the numerator alone: sum_q |w^ - w| |u(q)| (1 / N) <= (55 / 64) c'_G U max|u| (64 / 9).
That is (26 + (55 / 9) c'_G) U max|u| per level, below K'_G = 51 + (110 / 9) c'_G, the form of tests/test_gpu_denoise.py with c'_G in place of c_G, which is what is
asserted: |computed D_x u - D_x u| <= L K'_G U max|u| (a level's rows add up to 1 within a few U, so it passes earlier errors on unamplified to first order).
K'_0 = 119.1, K'_1 = 123.6, K'_8 = 137.1.  The transpose's bound is carried through the levels by the restatement, as `adjoint_bound` of tests/test_gpu_denoise.py does,
with the record's weights and 1 / N:  E <- A_l^T E + U ((51 + (55 / 9) c'_G) A_l^T t + (64 / 9) c'_G Hb_l t),  t <- A_l^T t,  from t = |y|, E = 0.
(A subnormal dl^2 or weight may be flushed to 0: an absolute error below 1e-25 in the argument, left out.)"""
import numpy as np
import pytest

import denoise_ref as dref
import scenes
import test_denoise_cpu as dcpu
import test_vdenoise_cpu as vcpu
import vdenoise_ref as ref

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
EPS = 1e-12
K_L = 0.25                                    # sigma_l = 2
SHAPES = [(1, 1), (1, 7), (5, 3), (32, 8), (33, 9), (64, 17), (67, 35)]
FULL = [(33, 9), (67, 35)]                    # the shapes that run every C and G
CASES = [(w, h, l, 3, 8) for (w, h) in SHAPES for l in (1, 3, 5)] + \
        [(w, h, l, c, g) for (w, h) in FULL for l in (1, 3, 5) for c in (1, 3) for g in (0, 1, 8) if (c, g) != (3, 8)]


def c_of(G):
    return ((max(G + 2, 7) + 1) if G else 7) / np.e + 3.0


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


def _cuda(env, a):
    return env[0].from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _denoiser(env, g, W, H, L, sigma_l=2.0):
    torch, psdr = env
    return psdr.VarianceDenoiser(torch.from_numpy(g) if g is not None and g.shape[1] else None, W, H, levels=L, sigma_l=sigma_l, eps=EPS)


def _case(W, H, L, C, G):
    rng = np.random.default_rng(W * 10000 + H * 100 + L * 10 + C + G)
    g = dcpu._guides(rng, W, H, G)
    x, v = vcpu._inputs(rng, W, H, C)
    return rng, g, x, v


def reference_tolerance(x, v, g, W, H, L, k=K_L):
    """(want, want_v, tolerance, tolerance_v) of the module docstring; NaN entries of want get a tolerance of NaN (the caller compares those by their own rule)"""
    want, want_v, _ = ref.apply(x, v, g, W, H, L, k, EPS)
    spread, spread_v = np.zeros_like(want), np.zeros_like(want_v)
    for seed in range(8):
        rng = np.random.default_rng(1000 + seed)
        nudge = lambda a: a.astype(np.float64) * (1.0 + rng.choice([-1.0, 1.0], a.shape) * 2.0 ** -23)          # noqa: E731
        o, ov, _ = ref.apply(nudge(x), nudge(v), nudge(g) if g is not None else None, W, H, L, k, EPS)
        with np.errstate(invalid="ignore"):
            spread, spread_v = np.maximum(spread, np.abs(o - want)), np.maximum(spread_v, np.abs(ov - want_v))
    fx, fv = np.abs(x[np.isfinite(x)]).max(), np.abs(v[np.isfinite(v)]).max()
    return want, want_v, 16 * np.maximum(spread, 4 * U * fx), 16 * np.maximum(spread_v, 4 * U * fv)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. apply against the restatement
@pytest.mark.parametrize("W,H,L,C,G", CASES)
def test_apply_against_the_restatement(env, W, H, L, C, G):
    _, g, x, v = _case(W, H, L, C, G)
    den = _denoiser(env, g, W, H, L)
    got = den(_cuda(env, x), _cuda(env, v)).cpu().numpy()
    got_v = den.variance.cpu().numpy()
    want, want_v, tol, tol_v = reference_tolerance(x, v, g, W, H, L)
    err, err_v = np.abs(got.astype(np.float64) - want), np.abs(got_v.astype(np.float64) - want_v)
    print("%d x %d, L %d, C %d, G %d: image error / tolerance %.3g, variance error / tolerance %.3g" % (W, H, L, C, G, (err / tol).max(), (err_v / tol_v).max()))
    assert got.shape == x.shape and got_v.shape == v.shape
    assert np.isfinite(got).all() and np.all(err <= tol), np.argwhere(err > tol)[:5]
    assert np.isfinite(got_v).all() and np.all(err_v <= tol_v), np.argwhere(err_v > tol_v)[:5]
    if W * H > 100:          # the luminance weight matters: the same image through the plain denoiser is not within the tolerance
        assert (np.abs(dref.apply(x, g, W, H, L) - want) > tol).any()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the frozen operator and its transpose against the restatement fed the device's record
def adjoint_bound(y, g, record, W, H, G):
    """E of the module docstring: [W H, C]"""
    t = np.abs(np.asarray(y, np.float64)).reshape(H, W, -1)
    E = np.zeros_like(t)
    c = c_of(G)
    for l in range(len(record) - 1, -1, -1):
        w, _ = ref.level_weights(g, record, K_L, EPS, W, H, l)
        w0, _ = dref.weights(None, W, H, l)
        inv = record[l][2][..., None]
        At = ref._gather(t * inv, w, W, H, l)
        E = ref._gather(E * inv, w, W, H, l) + U * ((51.0 + 55.0 / 9.0 * c) * At + 64.0 / 9.0 * c * ref._gather(t, w0, W, H, l))
        t = At
    return E.reshape(W * H, -1)


@pytest.mark.parametrize("W,H,L,C,G", CASES)
def test_frozen_and_transpose_against_the_restatement(env, W, H, L, C, G):
    rng, g, x, v = _case(W, H, L, C, G)
    den = _denoiser(env, g, W, H, L)
    den(_cuda(env, x), _cuda(env, v))
    rec = den.record().cpu().numpy()
    assert rec.shape == (L, 3, W * H) and np.isfinite(rec).all() and (rec[:, 2] <= np.float32(64.0 / 9.0)).all() and (rec[:, 1] >= 0).all()
    record = ref.record_planes(rec, W, H)
    Cu = 4 - C                                                                   # the other channel count: C of a frozen call need not be the recording's
    u = dcpu_image(rng, W * H, Cu)
    got, want = den.frozen(_cuda(env, u)).cpu().numpy(), ref.frozen(u, g, record, W, H, K_L, EPS)
    bound = L * k_of(G) * U * np.abs(u).max()
    err = np.abs(got.astype(np.float64) - want)
    got_t, want_t = den.frozen_transpose(_cuda(env, u)).cpu().numpy(), ref.frozen_adj(u, g, record, W, H, K_L, EPS)
    bound_t = adjoint_bound(u, g, record, W, H, G)
    err_t = np.abs(got_t.astype(np.float64) - want_t)
    print("%d x %d, L %d, C %d, G %d: frozen error / bound %.3g (bound %.3g); transpose error / bound %.3g" %
          (W, H, L, Cu, G, err.max() / bound, bound, (err_t / np.maximum(bound_t, 1e-300)).max()))
    assert got.shape == u.shape and np.isfinite(got).all() and np.all(err <= bound), np.argwhere(err > bound)[:5]
    assert np.isfinite(got_t).all() and np.all(err_t <= bound_t), np.argwhere(err_t > bound_t)[:5]


def dcpu_image(rng, n, C):
    """both signs, magnitudes over four decades (the image of tests/test_gpu_denoise.py)"""
    return (rng.standard_normal((n, C)) * 10.0 ** rng.uniform(-2, 2, (n, 1))).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the transpose identity
@pytest.mark.parametrize("W,H,L,C,G", [(33, 9, 5, 3, 8), (67, 35, 5, 3, 8), (67, 35, 3, 1, 1), (64, 17, 5, 3, 0), (5, 3, 3, 3, 8)])
def test_transpose_identity(env, W, H, L, C, G):
    """<D_x u, y> and <u, D_x^T y> in float64 from the device results agree within twice the relative bound of test 2, L K'_G U, times sum |u| |y|"""
    rng, g, x, v = _case(W, H, L, C, G)
    den = _denoiser(env, g, W, H, L)
    den(_cuda(env, x), _cuda(env, v))
    u, y = rng.standard_normal((W * H, C)).astype(np.float32), rng.standard_normal((W * H, C)).astype(np.float32)
    lhs = float((den.frozen(_cuda(env, u)).cpu().numpy().astype(np.float64) * y).sum())
    rhs = float((u.astype(np.float64) * den.frozen_transpose(_cuda(env, y)).cpu().numpy()).sum())
    tol = 2 * L * k_of(G) * U * float((np.abs(u).astype(np.float64) * np.abs(y)).sum())
    print("%d x %d, L %d, C %d, G %d: %.9g against %.9g, difference %.3g, bound %.3g" % (W, H, L, C, G, lhs, rhs, abs(lhs - rhs), tol))
    assert abs(lhs - rhs) <= tol


# ---------------------------------------------------------------------------------------------------------------------------
# 4. sigma_l = inf is the plain denoiser
@pytest.mark.parametrize("W,H,L,C,G", [(33, 9, 5, 3, 8), (67, 35, 5, 3, 0), (5, 3, 3, 1, 1)])
def test_infinite_sigma_gives_the_denoisers_bits(env, W, H, L, C, G):
    torch, psdr = env
    _, g, x, v = _case(W, H, L, C, G)
    gt = torch.from_numpy(g) if G else None
    plain = psdr.Denoiser(gt, W, H, levels=L)(_cuda(env, x))
    den = psdr.VarianceDenoiser(gt, W, H, levels=L, sigma_l=float("inf"), eps=EPS)
    got = den(_cuda(env, x), _cuda(env, v))
    assert den.k == 0.0 and torch.equal(got, plain)
    assert not torch.equal(_denoiser(env, g, W, H, L)(_cuda(env, x), _cuda(env, v)), plain)          # and sigma_l = 2 is another filter


# ---------------------------------------------------------------------------------------------------------------------------
# 5. bit equalities
def test_bit_equalities_and_autograd(env):
    torch, psdr = env
    W, H, L, C, G = 67, 35, 5, 3, 8
    rng, g, x, v = _case(W, H, L, C, G)
    den = _denoiser(env, g, W, H, L)
    xt, vt = _cuda(env, x), _cuda(env, v)
    gy = _cuda(env, dcpu_image(rng, W * H, C))
    with pytest.raises(RuntimeError, match="no record"):
        den.frozen(xt)
    with pytest.raises(RuntimeError, match="no record"):
        den.frozen_transpose(xt)
    a = den(xt, vt)
    va = den.variance
    assert torch.equal(den.frozen(xt), a)                                        # the record reproduces the apply
    b = den(xt, vt)
    assert torch.equal(a, b) and torch.equal(va, den.variance) and not den.variance.requires_grad
    ta, tb = den.frozen_transpose(gy), den.frozen_transpose(gy)
    assert torch.equal(ta, tb)
    again = _denoiser(env, g, W, H, L)                                           # another handle from the same inputs
    assert torch.equal(again(xt, vt), a) and torch.equal(again.frozen_transpose(gy), ta)
    img = xt.clone().requires_grad_()
    var = vt.clone().requires_grad_()
    out = den(img, var)
    assert out.requires_grad and torch.equal(out.detach(), a)
    out.backward(gy)
    assert torch.equal(img.grad, ta) and var.grad is None
    # a second apply replaces the record: other inputs, another operator, and it is the new one that frozen applies
    x2, v2 = vcpu._inputs(np.random.default_rng(99), W, H, C)
    a2 = den(_cuda(env, x2), _cuda(env, v2))
    assert torch.equal(den.frozen(_cuda(env, x2)), a2) and not torch.equal(den.frozen(xt), a)
    assert not torch.equal(den.frozen_transpose(gy), ta)
    # a backward whose record has been replaced is refused, not answered with the wrong operator
    img2 = xt.clone().requires_grad_()
    out2 = den(img2, vt)
    den(_cuda(env, x2), _cuda(env, v2))
    with pytest.raises(RuntimeError, match="replaced the record"):
        out2.backward(gy)
    # a float64 image: made float32 on the way in, the gradient goes back in the input's type; one channel after three
    leaf = xt.double().requires_grad_()
    den(leaf, vt.reshape(-1, 1)).backward(gy)
    assert leaf.grad.dtype == torch.float64 and torch.equal(leaf.grad, ta.double())
    assert tuple(den.frozen(xt[:, :1].contiguous()).shape) == (W * H, 1)
    for bad in (torch.zeros((W * H, 2), device="cuda"), torch.zeros((W * H, 4), device="cuda"), torch.zeros((W * H + 1, 3), device="cuda")):
        with pytest.raises(ValueError, match="expected"):
            den(bad, vt)
    with pytest.raises(ValueError, match="variance"):
        den(xt, vt[:-1])
    with pytest.raises(ValueError, match="luminance"):
        psdr.VarianceDenoiser(None, W, H, luminance=(1.0,))(xt, vt)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the non-finite rule
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("what", ["x", "guide", "v"])
@pytest.mark.parametrize("where", ["interior", "corner"])
def test_non_finite_rule(env, bad, what, where):
    """a non-finite x or guide at q cuts q off, a non-finite v the pixels of q's 3 x 3 unit neighbourhood: the output is finite away from q and within test 1's tolerance
    of the restatement (which states the rule); q's value reaches no other pixel (another value at q changes the output at q alone, bit for bit) and q's own centre tap
    hands its value through"""
    W, H, L, G, C = 33, 9, 3, 3, 3
    rng = np.random.default_rng(17)
    g = dcpu._guides(rng, W, H, G) * np.float32(0.1)
    x = (1.0 + 0.1 * rng.standard_normal((W * H, C))).astype(np.float32)
    v = np.full(W * H, 0.5, dtype=np.float32)
    qx, qy = (20, 4) if where == "interior" else (0, 0)
    q = qy * W + qx
    if what == "x":
        x[q, 1] = bad
    elif what == "guide":
        g[q, 1] = bad
    else:
        v[q] = bad
    den = _denoiser(env, g, W, H, L)
    got = den(_cuda(env, x), _cuda(env, v)).cpu().numpy()
    got_v = den.variance.cpu().numpy()
    want, want_v, tol, tol_v = reference_tolerance(x, v, g, W, H, L)
    others = np.arange(W * H) != q
    assert np.isfinite(got[others]).all() and np.isfinite(got_v[others]).all()
    assert np.all(np.abs(got[others] - want[others]) <= tol[others]) and np.all(np.abs(got_v[others] - want_v[others]) <= tol_v[others])
    assert np.array_equal(np.isfinite(got[q]), np.isfinite(x[q])) and np.isfinite(got_v[q]) == np.isfinite(v[q])
    fin = np.isfinite(x[q])
    assert np.all(np.abs(got[q][fin].astype(np.float64) - x[q][fin]) <= L * 51 * U * np.abs(x[q][fin]))          # every level hands q back: x h(0)^2 / h(0)^2
    x2 = x.copy()
    x2[q] = [1.0e3, -2.0e3, 5.0e2] if what != "x" else [1.0e3, bad, 5.0e2]
    got2 = den(_cuda(env, x2), _cuda(env, v)).cpu().numpy()
    assert np.array_equal(got[others], got2[others]) and not np.array_equal(got[q][fin], got2[q][fin])
    # the frozen operator and its transpose keep what they are given finite
    u = dcpu_image(rng, W * H, C)
    assert np.isfinite(den.frozen(_cuda(env, u)).cpu().numpy()).all() and np.isfinite(den.frozen_transpose(_cuda(env, u)).cpu().numpy()).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 7. the step frames: what the feature is for
@pytest.mark.parametrize("seed", range(4))
def test_step_frames_keep_the_illumination_edge(env, seed):
    """64 x 48, a luminance step 0.2 | 1.0 across a slanted line, no guide edge (G = 0), L = 5, sigma_l = 2.  With the exact variance of 10 % relative noise the float64
    prototype leaves MSE(out) / MSE(noisy) = 0.0133, 0.0110, 0.0097, 0.0123 (seeds 0..3) where psdr.Denoiser leaves 10.5: it wipes the edge out, and this test fails
    without the luminance weight.  With a variance estimated from two samples at 30 % noise: 0.053, 0.063, 0.052, 0.062.  The caps, 1/40 and 1/8, are about twice the
    prototype's figures; tests/test_vdenoise_cpu.py re-measures them on the restatement."""
    torch, psdr = env
    noisy, v, clean = vcpu.step_exact(seed)
    den = psdr.VarianceDenoiser(None, vcpu.SW, vcpu.SH, levels=5, sigma_l=2.0)
    out = den(_cuda(env, noisy), _cuda(env, v)).cpu().numpy()
    plain = psdr.Denoiser(None, vcpu.SW, vcpu.SH, levels=5)(_cuda(env, noisy)).cpu().numpy()
    r, r_plain = vcpu.mse(out, clean) / vcpu.mse(noisy, clean), vcpu.mse(plain, clean) / vcpu.mse(noisy, clean)
    mean, ve, _ = vcpu.step_estimated(seed)
    r_est = vcpu.mse(den(_cuda(env, mean), _cuda(env, ve)).cpu().numpy(), clean) / vcpu.mse(mean, clean)
    print("seed %d: exact variance %.4f (prototype %.4f), Denoiser %.2f x the noisy error, estimated variance %.4f (prototype %.3f)" %
          (seed, r, vcpu.PROTOTYPE_EXACT[seed], r_plain, r_est, vcpu.PROTOTYPE_ESTIMATED[seed]))
    assert r <= 1.0 / 40.0
    assert r_plain > 5.0
    assert r_est <= 1.0 / 8.0


def test_luminance_variance_on_the_device(env):
    torch, psdr = env
    rng = np.random.default_rng(5)
    n = 4
    smp = rng.uniform(0.0, 2.0, (n, 50, 3))
    mean, sq = (smp / n).sum(axis=0), ((smp / n) ** 2).sum(axis=0)
    want = (np.array(ref.REC709) * np.sqrt(smp.var(axis=0, ddof=1) / n)).sum(axis=1) ** 2
    got = psdr.luminance_variance(_cuda(env, mean), _cuda(env, sq), n)
    assert tuple(got.shape) == (50,) and got.dtype == torch.float32
    assert np.abs(got.cpu().numpy() - want).max() <= 1e-4 * want.max()          # (sq - mean^2 / n cancels a few digits in float32)


# ---------------------------------------------------------------------------------------------------------------------------
# 8. end to end
W8 = H8 = 32
LOW_SPP, TRUTH_SPP = 2, 1024


def _set_spp(sc, spp):
    sc.opts.spp = spp
    sc.configure(sc.__dict__.get("_psdr_active", []))


def test_denoised_low_spp_render_is_closer_to_the_truth(env):
    """The 32 x 32 Cornell box of tests/test_gpu_denoise.py: render_c_sq at 2 spp (seed 5) against renderC at 1024 spp (seed 11), guides from seed 3, L = 5, sigma_l = 2,
    the variance by luminance_variance.  Measured first on the CPU - the oracle's per-lane radiances of the same scene with the same seeds give the image and the sums of
    squares, its field renders scaled by first_hit_guides' rule the guides, all put through tests/vdenoise_ref.py - at spp 2, 4, 8 in that order:

        spp   MSE(noisy)   MSE(denoised)   ratio     psdr.Denoiser's ratio on the same frame
        2     0.13396      0.070932        0.530     0.426
        4     0.076406     0.056078        0.734     0.593
        8     0.020391     0.012881        0.632     0.517

    2 spp is the first whose ratio is below 0.8, so that is the case run here, and the assertion is the plain inequality.  On this frame the plain denoiser is ahead at
    every spp (why has not been looked into; a variance estimated from two to eight samples is itself very noisy, and a firefly with a large estimate is kept as if it
    were an edge); the step frames of test 7 are where the variance weight pays.  Denoiser's ratio is printed and nothing is asserted about it."""
    import product
    torch, psdr = env
    sc = product.build_scene(scenes.cbox_scene(W8, H8, spp=LOW_SPP, param=None))
    integ = psdr.PathTracer(2)
    guides = psdr.first_hit_guides(sc, seed=3)
    den = psdr.VarianceDenoiser(guides, W8, H8, levels=5, sigma_l=2.0)
    noisy, sq = psdr.render_c_sq(integ, sc, 0, seed=5)
    v = psdr.luminance_variance(noisy, sq, psdr.samples_behind(sc, psdr.TERM_INTERIOR))
    try:
        _set_spp(sc, TRUTH_SPP)
        truth = integ.renderC(sc, 0, seed=11)
    finally:
        _set_spp(sc, LOW_SPP)
    out = den(noisy, v)
    plain = psdr.Denoiser(guides, W8, H8, levels=5)(noisy)
    mse_noisy, mse_den, mse_plain = float(((noisy - truth) ** 2).mean()), float(((out - truth) ** 2).mean()), float(((plain - truth) ** 2).mean())
    print("MSE against %d spp: %d spp %.5g, denoised %.5g, ratio %.3f; psdr.Denoiser %.5g, ratio %.3f" %
          (TRUTH_SPP, LOW_SPP, mse_noisy, mse_den, mse_den / mse_noisy, mse_plain, mse_plain / mse_noisy))
    assert tuple(v.shape) == (W8 * H8,) and bool((v >= 0).all()) and float(v.max()) > 0
    assert mse_noisy > 0 and mse_den < mse_noisy


def test_backward_through_the_denoiser_is_the_frozen_transpose(env):
    """loss(den(renderD(...), v)).backward(): the gradient that reaches the render is den.frozen_transpose(dloss / dout), the same tensor bit for bit - that is all of the
    denoiser's part.  (The leaf gradient behind the render is not bit-reproducible, its reverse pass adds with float atomics; tests/test_gpu_denoise.py states and
    bounds that.)  v comes from render_c_sq of the same scene and gets no gradient."""
    torch, psdr = env
    from test_gpu_adaptive import _moving_box_scene
    width, height, spp = 32, 32, 2
    P = psdr.FloatD(0.).requires_grad_()
    sc = _moving_box_scene(psdr, P, width, height, spp)
    integ = psdr.PathTracer(2)
    mean, sq = psdr.render_c_sq(integ, sc, 0, seed=7)
    v = psdr.luminance_variance(mean, sq, psdr.samples_behind(sc, psdr.TERM_INTERIOR))
    den = psdr.VarianceDenoiser(psdr.first_hit_guides(sc, seed=3), width, height, levels=5)
    w = torch.linspace(0.5, 1.5, width * height * 3, device="cuda").reshape(-1, 3)
    seen = []
    img = integ.renderD(sc, 0, seed=7)
    img.register_hook(lambda grad: seen.append(grad.clone()))
    (den(img, v) * w).sum().backward()
    by_hand = den.frozen_transpose(w)
    assert len(seen) == 1 and torch.equal(seen[0], by_hand)
    assert P.grad is not None and bool(torch.isfinite(P.grad).all()) and float(by_hand.abs().max()) > 0
